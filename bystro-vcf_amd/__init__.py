"""bystro-vcf_amd — Python binding of libbvcf.so (the MI355X-native per-line variant pipeline).

This package is plumbing for tests and benchmarks: every call goes through the C-ABI declared in
include/bvcf.h.  There is no Python or CPU implementation of the path here; if the HIP library is
missing the import fails.
"""
import ctypes as C
import os

import numpy as np

# One HIP runtime per process: torch bundles its own libamdhip64 (same SONAME as /opt/rocm's).
# Loading torch first makes libbvcf.so bind to that copy instead of pulling in a second runtime,
# which would leave the later one without a usable device.
try:
    import torch  # noqa: F401
except ImportError:  # the library then binds to /opt/rocm's runtime through its RUNPATH
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BVCF_LIB") or os.path.join(_HERE, "libbvcf.so")  # BVCF_LIB: A/B another build

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "bystro-vcf_amd: %s not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C bystro-vcf_amd/csrc`); there is no fallback path" % LIB_PATH)

lib = C.CDLL(LIB_PATH)

ABI_VERSION = 9
ABI_VERSION_SUBSET = 10  # bvcf_params.abi_version of a ctx that is to read sample_keep (BVCF_ABI_VERSION_SUBSET)
DEVICE_PAD = 64
NO_CMAP = 0xFFFFFFFF

OK, E_ARG, E_HIP, E_NODEV, E_BUSY, E_EMPTY, E_TOO_BIG, E_CAPACITY, E_NOMEM, E_FATAL = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9
LINE_OK, LINE_FIELDS, LINE_FILTER, LINE_NOALLELE = 0, 1, 2, 3
ALLELE_POS_TEXT = 1  # BVCF_ALLELE_POS_TEXT in bvcf_allele.flags: the output pos is the POS field verbatim, the record's pos is 0
SITE_NAMES = ["SNP", "INS", "DEL", "MNP", "MULTIALLELIC"]
ALT_BASE, ALT_INS, ALT_DEL = 0, 1, 2
CLS_NONE, CLS_HET, CLS_HOM, CLS_MISSING = 0, 1, 2, 3
# the header line of the --sampleStats table (bvcf_config.sample_stats_path)
SAMPLE_STATS_COLUMNS = ["sample", "het", "hom", "missing", "transitions", "transversions", "heterozygosity", "homozygosity",
                        "missingness", "trTv"]
# the header line of the --relatedness table (bvcf_config_more.pair_stats_path): one line per unordered pair of samples
PAIR_STATS_COLUMNS = ["sample1", "sample2", "hetHet", "ibs0", "het1", "het2", "kinship"]
PAIR_MAX_SAMPLES = 8192  # BVCF_PAIR_MAX_SAMPLES

# the measurement hooks of include/bvcf_bench.h (not part of the drop-in ABI)
BENCH_EXPORTS = ["bvcf_bench_device", "bvcf_bench_device_slots", "bvcf_bench_stream_kernel", "bvcf_bench_head_left",
                 "bvcf_bench_pair_kernels", "bvcf_bench_grm_kernels", "bvcf_bench_score_kernels", "bvcf_bench_assoc_kernels", "bvcf_bench_assoc_cov_kernels", "bvcf_bench_assoc_logit_kernels", "bvcf_bench_hwe", "bvcf_bench_gate_kernels", "bvcf_bench_bed_kernels",
                 "bvcf_bench_deflate_codes", "bvcf_bench_trio_kernels", "bvcf_bench_ld_kernels",
                 "bvcf_bench_variant_kernel", "bvcf_bench_variant_gate_stride",
                 "bvcf_bench_region_kernel", "bvcf_bench_region_gate_stride",
                 "bvcf_bench_pca_eigen", "bvcf_bench_guard_check", "bvcf_bench_guarded_buffers"]

# the partition logic of bvcf_run_fd, exported for host-only tests (include/bvcf_plan.h; not part of the drop-in ABI)
PLAN_EXPORTS = ["bvcf_plan_text_ranges", "bvcf_plan_bgzf_ranges", "bvcf_cut_text_range", "bvcf_find_bgzf_chain",
                "bvcf_plan_threads", "bvcf_plan_fd", "bvcf_head_fast_line", "bvcf_plan_ctx",
                "bvcf_site_gate_verdict", "bvcf_hwe_exact", "bvcf_hwe_inline_terms", "bvcf_bed_row",
                "bvcf_trio_verdict", "bvcf_parse_fam",
                "bvcf_ld_counts", "bvcf_ld_in_ld", "bvcf_parse_ld_r2", "bvcf_ld_seam_create", "bvcf_ld_seam_push",
                "bvcf_ld_seam_read", "bvcf_ld_seam_rows", "bvcf_ld_seam_pairs", "bvcf_ld_seam_destroy",
                "bvcf_score_weight", "bvcf_score_limbs", "bvcf_score_decimal",
                "bvcf_assoc_value", "bvcf_assoc_limbs", "bvcf_assoc_ints", "bvcf_pca_tridiag"]

# every symbol include/bvcf.h declares
EXPORTS = [
    "bvcf_create", "bvcf_destroy", "bvcf_last_error", "bvcf_version", "bvcf_reserve", "bvcf_set_sample_names", "bvcf_set_row_format", "bvcf_alloc_pinned", "bvcf_alloc_pinned_near", "bvcf_warmup",
    "bvcf_free_pinned", "bvcf_submit", "bvcf_submit_device", "bvcf_submit_bgzf", "bvcf_collect", "bvcf_sample_stats", "bvcf_enable_pair_stats", "bvcf_pair_stats", "bvcf_counters", "bvcf_sum_counters",
    "bvcf_allreduce_counters", "bvcf_device_count", "bvcf_device_pci_bus_id", "bvcf_path", "bvcf_config_defaults", "bvcf_config_more_defaults", "bvcf_string_header", "bvcf_format_tsv", "bvcf_run_buffer", "bvcf_run_fd", "bvcf_decompress_fd", "bvcf_bgzf_inflate_device", "bvcf_bgzf_deflate_device", "bvcf_free",
    "bvcf_arrow_open", "bvcf_arrow_append", "bvcf_arrow_close",
    "bvcf_site_gate_defaults", "bvcf_set_site_gate", "bvcf_site_gate_count", "bvcf_config_gate_defaults",
    "bvcf_enable_bed_rows", "bvcf_reserve_bed_rows", "bvcf_bed_rows", "bvcf_config_plink_defaults",
    "bvcf_enable_trios", "bvcf_reserve_trio_events", "bvcf_trio_stats", "bvcf_config_trios_defaults",
    "bvcf_enable_ld", "bvcf_reserve_ld_events", "bvcf_ld_stats", "bvcf_config_ld_defaults",
    "bvcf_locus_hash", "bvcf_variant_table_capacity", "bvcf_variant_table_build", "bvcf_variant_table_parse",
    "bvcf_variant_table_free", "bvcf_variant_table_has", "bvcf_set_variant_table", "bvcf_set_variant_list",
    "bvcf_variant_gate_count", "bvcf_config_variants_defaults",
    "bvcf_region_table_parse_specs", "bvcf_region_table_parse_bed", "bvcf_region_table_build", "bvcf_region_table_free",
    "bvcf_region_table_has", "bvcf_region_table_stays", "bvcf_set_region_table", "bvcf_region_gate_count",
    "bvcf_config_regions_defaults",
    "bvcf_enable_grm", "bvcf_grm", "bvcf_config_grm_defaults",
    "bvcf_score_table_build", "bvcf_score_table_parse", "bvcf_score_table_free", "bvcf_score_table_find", "bvcf_set_score_table",
    "bvcf_score", "bvcf_config_score_defaults",
    "bvcf_pheno_table_build", "bvcf_pheno_table_parse", "bvcf_pheno_table_free", "bvcf_set_pheno_table",
    "bvcf_reserve_assoc_rows", "bvcf_assoc", "bvcf_assoc_stat", "bvcf_config_assoc_defaults",
    "bvcf_grm_matrix", "bvcf_pca_eigen", "bvcf_config_pca_defaults",
    "bvcf_covar_table_parse", "bvcf_covar_table_build", "bvcf_covar_table_free", "bvcf_pheno_table_mask", "bvcf_set_covar_table",
    "bvcf_assoc_cov", "bvcf_assoc_cov_stat", "bvcf_config_covar_defaults",
    "bvcf_logit_table_build", "bvcf_logit_table_free", "bvcf_set_logit_table", "bvcf_assoc_logit", "bvcf_assoc_logit_stat",
    "bvcf_config_logit_defaults",
]


class Params(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("device", C.c_int32), ("n_header_fields", C.c_uint32),
        ("eol_chars", C.c_uint32), ("eol_byte", C.c_uint8), ("want_class_maps", C.c_uint8),
        ("want_dosage", C.c_uint8), ("want_name_lists", C.c_uint8), ("allow_filter", C.c_char_p), ("exclude_filter", C.c_char_p),
        ("max_batch_bytes", C.c_uint64), ("max_lines", C.c_uint32), ("max_alleles", C.c_uint32),
        ("cmap_bytes", C.c_uint64), ("n_slots", C.c_uint32), ("path", C.c_uint32),
        ("packed_sites", C.c_uint32), ("render_sites", C.c_uint32), ("want_sample_stats", C.c_uint32),
        ("min_gq", C.c_uint32), ("min_dp", C.c_uint32), ("sample_keep", C.POINTER(C.c_uint32)),
    ]


class Config(C.Structure):
    _fields_ = [
        ("empty_field", C.c_char_p), ("field_delimiter", C.c_char_p), ("allow_filter", C.c_char_p),
        ("exclude_filter", C.c_char_p), ("keep_id", C.c_uint8), ("keep_info", C.c_uint8),
        ("keep_pos", C.c_uint8), ("keep_qual", C.c_uint8), ("normalize_header", C.c_uint8),
        ("leave_teardown_to_exit", C.c_uint8), ("reserved", C.c_uint8 * 2), ("device", C.c_int32), ("n_format_threads", C.c_uint32),
        ("max_batch_bytes", C.c_uint64), ("sample_list_path", C.c_char_p),
        ("dosage_path", C.c_char_p), ("no_out", C.c_uint8), ("out_bgzf", C.c_uint8), ("reserved3", C.c_uint8 * 2),
        ("n_devices", C.c_uint32), ("devices", C.POINTER(C.c_int32)), ("sample_stats_path", C.c_char_p),
        ("min_gq", C.c_uint32), ("min_dp", C.c_uint32),
        ("keep_samples_path", C.c_char_p), ("exclude_samples_path", C.c_char_p),
    ]


CONFIG_MORE = 1  # BVCF_CONFIG_MORE in Config.reserved[0]: the struct is the head of a ConfigMore


CONFIG_MORE_GATE = 1  # BVCF_CONFIG_MORE_GATE in Config.reserved[1]: the ConfigMore reaches up to site_filter_path
# bvcf_allele.pad[0] of a row the site gate took out: the criteria it fails
GATE_MIN_MAF, GATE_MAX_MAF, GATE_MIN_MAC, GATE_MAX_MISSING, GATE_HWE = 1, 2, 4, 8, 16
# the lines of the --siteFilterReport file, and of site_gate_count()
SITE_GATE_REPORT = ["examined", "kept", "minMaf", "maxMaf", "minMac", "maxMissing", "hwe"]


class SiteGate(C.Structure):
    """bvcf_site_gate"""
    _fields_ = [("size", C.c_uint32), ("min_mac", C.c_uint32), ("min_maf", C.c_double), ("max_maf", C.c_double),
                ("max_missing", C.c_double), ("hwe_p", C.c_double)]


def make_site_gate(minMaf=0.0, maxMaf=1.0, minMac=0, maxMissing=1.0, hwe=0.0):
    """a bvcf_site_gate from the CLI's names; the defaults are the neutral values"""
    g = SiteGate()
    lib.bvcf_site_gate_defaults(C.byref(g))
    g.min_maf, g.max_maf, g.min_mac, g.max_missing, g.hwe_p = float(minMaf), float(maxMaf), int(minMac), float(maxMissing), float(hwe)
    return g


GATE_KEYS = ("minMaf", "maxMaf", "minMac", "maxMissing", "hwe")


CONFIG_MORE_PLINK = 2  # BVCF_CONFIG_MORE_PLINK in Config.reserved[1]: ... up to plink_prefix (and so the gate fields too)
BED_MAGIC = b"\x6c\x1b\x01"  # a variant-major PLINK 1 .bed
# class -> .bed code with A1 = the row's ALT: none 3 (hom A2), het 2, hom 0 (hom A1), missing 1
BED_CODE = (3, 2, 0, 1)


class BedRowsInfo(C.Structure):
    """bvcf_bed_rows_info"""
    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_uint64), ("row_bytes", C.c_uint32), ("reserved", C.c_uint32),
                ("need_bytes", C.c_uint64)]


class ConfigMore(C.Structure):
    """bvcf_config_more: bvcf_config and the fields that came after it stopped growing"""
    _fields_ = [("base", Config), ("pair_stats_path", C.c_char_p), ("site_gate", SiteGate), ("site_filter_path", C.c_char_p),
                ("plink_prefix", C.c_char_p)]


CONFIG_MORE_TRIOS = 3  # BVCF_CONFIG_MORE_TRIOS in Config.reserved[1]: the ConfigMore is the head of a ConfigTrios
# bvcf_trio_verdict / BVCF_TRIO_*; the classes it takes are the class maps': none 0, het 1, hom 2, missing 3
TRIO_UNINFORMATIVE, TRIO_CONSISTENT, TRIO_DENOVO, TRIO_ERROR = 0, 1, 2, 3
# bvcf_parse_fam / BVCF_FAM_*
FAM_OK, FAM_SHORT_LINE, FAM_DUP_IID, FAM_AMBIGUOUS, FAM_SAME_SAMPLE = 0, 1, 2, 3, 4
MENDEL_COLUMNS = ["child", "father", "mother", "informative", "errors", "denovo", "errorRate"]
MENDEL_ERRORS_COLUMNS = ["chrom", "pos", "ref", "alt", "child", "father", "mother", "childClass", "fatherClass", "motherClass",
                         "kind"]


class ConfigTrios(C.Structure):
    """bvcf_config_trios: a bvcf_config_more and the paths that came after it stopped growing"""
    _fields_ = [("more", ConfigMore), ("fam_path", C.c_char_p), ("mendel_path", C.c_char_p), ("mendel_errors_path", C.c_char_p)]


class TrioInfo(C.Structure):
    """bvcf_trio_info"""
    _fields_ = [("counts", C.c_void_p), ("events", C.c_void_p), ("n_events", C.c_uint64), ("need_events", C.c_uint64),
                ("n_trios", C.c_uint32), ("reserved", C.c_uint32)]


CONFIG_MORE_LD = 4  # BVCF_CONFIG_MORE_LD in Config.reserved[1]: the ConfigTrios is the head of a ConfigLd
LD_COLUMNS = ["chrom", "pos1", "ref1", "alt1", "pos2", "ref2", "alt2", "n", "r2", "dir"]
LD_MAX_WINDOW = 512


class ConfigLd(C.Structure):
    """bvcf_config_ld: a bvcf_config_trios and what came after it"""
    _fields_ = [("trios", ConfigTrios), ("ld_path", C.c_char_p), ("ld_prune_prefix", C.c_char_p), ("ld_window", C.c_uint32),
                ("ld_t6", C.c_uint32), ("ld_t6_set", C.c_uint32), ("reserved", C.c_uint32)]


CONFIG_MORE_VARIANTS = 5  # BVCF_CONFIG_MORE_VARIANTS in Config.reserved[1]: the ConfigLd is the head of a ConfigVariants
VARIANT_MAX_ENTRIES = 1 << 27  # BVCF_VARIANT_MAX_ENTRIES
# the lines of the --variantFilterReport file; variant_gate_count() gives the last three
VARIANT_REPORT = ["listed", "examined", "kept", "dropped"]
VARIANT_ENTRY_DTYPE = np.dtype([("tag", "<u4"), ("off", "<u4"), ("len", "<u4"), ("zero", "<u4")])


class ConfigVariants(C.Structure):
    """bvcf_config_variants: a bvcf_config_ld and what came after it"""
    _fields_ = [("ld", ConfigLd), ("keep_variants_path", C.c_char_p), ("exclude_variants_path", C.c_char_p),
                ("variant_filter_path", C.c_char_p)]


class VariantTableStruct(C.Structure):
    """bvcf_variant_table"""
    _fields_ = [("entries", C.c_void_p), ("capacity", C.c_uint64), ("blob", C.c_void_p), ("blob_bytes", C.c_uint64),
                ("n", C.c_uint64)]


def locus_hash(s):
    """bvcf_locus_hash: the 64-bit hash of a locus string (bytes) that places it in the table  (host code, no device)"""
    lib.bvcf_locus_hash.restype = C.c_uint64
    lib.bvcf_locus_hash.argtypes = [C.c_char_p, C.c_size_t]
    return int(lib.bvcf_locus_hash(bytes(s), len(s)))


def variant_table_capacity(n):
    """bvcf_variant_table_capacity: the slots of a table of n distinct entries (0 above VARIANT_MAX_ENTRIES)"""
    lib.bvcf_variant_table_capacity.restype = C.c_uint64
    lib.bvcf_variant_table_capacity.argtypes = [C.c_uint64]
    return int(lib.bvcf_variant_table_capacity(n))


class VariantTable:
    """a host table of locus strings: bvcf_variant_table_build over a list of bytes, or -- text= -- bvcf_variant_table_parse
    over the bytes of a list file  (host code, no device)"""

    def __init__(self, loci=None, text=None):
        self.t = VariantTableStruct()
        if text is not None:
            lib.bvcf_variant_table_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
            rc = lib.bvcf_variant_table_parse(bytes(text), len(text), C.byref(self.t))
        else:
            loci = [bytes(x) for x in loci]
            blob = b"".join(loci)
            lens = np.array([len(x) for x in loci], dtype=np.uint32)
            offs = np.zeros(len(loci), dtype=np.uint64)
            if len(loci) > 1:
                offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
            lib.bvcf_variant_table_build.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
            rc = lib.bvcf_variant_table_build(blob, offs.ctypes.data if len(loci) else None,
                                              lens.ctypes.data if len(loci) else None, len(loci), C.byref(self.t))
        if rc:
            raise BvcfError(rc, "bvcf_variant_table_build")

    @property
    def n(self):
        return int(self.t.n)

    @property
    def capacity(self):
        return int(self.t.capacity)

    @property
    def blob(self):
        return C.string_at(self.t.blob, self.t.blob_bytes) if self.t.blob_bytes else b""

    @property
    def entries(self):
        """the slots as a VARIANT_ENTRY_DTYPE array (copied)"""
        n = self.capacity * VARIANT_ENTRY_DTYPE.itemsize
        return np.frombuffer(C.string_at(self.t.entries, n), dtype=VARIANT_ENTRY_DTYPE).copy()

    def has(self, s):
        """bvcf_variant_table_has: the probe the device runs"""
        lib.bvcf_variant_table_has.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        r = lib.bvcf_variant_table_has(C.byref(self.t), bytes(s), len(s))
        if r < 0:
            raise ValueError("bvcf_variant_table_has: bad arguments")
        return bool(r)

    def close(self):
        lib.bvcf_variant_table_free.argtypes = [C.c_void_p]
        lib.bvcf_variant_table_free(C.byref(self.t))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CONFIG_MORE_REGIONS = 6  # BVCF_CONFIG_MORE_REGIONS in Config.reserved[1]: the ConfigVariants is the head of a ConfigRegions
REGION_MAX_INTERVALS = 1 << 26  # BVCF_REGION_MAX_INTERVALS
REGION_MAX_CHROMS = 1 << 20  # BVCF_REGION_MAX_CHROMS
# the lines of the --regionFilterReport file; region_gate_count() gives the last three
REGION_REPORT = ["keepIntervals", "excludeIntervals", "examined", "kept", "dropped"]
REGION_CHROM_DTYPE = np.dtype([("tag", "<u4"), ("off", "<u4"), ("len", "<u4"), ("zero", "<u4"), ("first", "<u4", (2,)),
                               ("n", "<u4", (2,))])
REGION_INTERVAL_DTYPE = np.dtype([("beg", "<i8"), ("end", "<i8")])
REGION_CONFIG_KEYS = (("regions", "regions"), ("regionsFile", "regions_path"), ("excludeRegions", "exclude_regions"),
                      ("excludeRegionsFile", "exclude_regions_path"), ("regionFilterReport", "region_filter_path"))


class ConfigRegions(C.Structure):
    """bvcf_config_regions: a bvcf_config_variants and what came after it"""
    _fields_ = [("variants", ConfigVariants), ("regions", C.c_char_p), ("regions_path", C.c_char_p),
                ("exclude_regions", C.c_char_p), ("exclude_regions_path", C.c_char_p), ("region_filter_path", C.c_char_p)]


CONFIG_MORE_GRM = 7  # BVCF_CONFIG_MORE_GRM in Config.reserved[1]: the ConfigRegions is the head of a ConfigGrm
GRM_MAX_BATCH_ROWS = 524288  # BVCF_GRM_MAX_BATCH_ROWS: most allele slots of a ctx with grm=True
GRM_SHIFT = 14  # the GRM's scores are in units of 2^-14: A = T / (2^28 N)


class ConfigGrm(C.Structure):
    """bvcf_config_grm: a bvcf_config_regions and what came after it"""
    _fields_ = [("regions", ConfigRegions), ("grm_prefix", C.c_char_p)]


CONFIG_MORE_SCORE = 8  # BVCF_CONFIG_MORE_SCORE in Config.reserved[1]: the ConfigGrm is the head of a ConfigScore
SCORE_ONE = 10 ** 12  # a weight's integer W is in units of 10^-12
SCORE_MAX_W = 10 ** 18
SCORE_MAX_COLUMNS = 64


class ConfigScore(C.Structure):
    """bvcf_config_score: a bvcf_config_grm and what came after it"""
    _fields_ = [("grm", ConfigGrm), ("score_path", C.c_char_p), ("score_output_path", C.c_char_p),
                ("score_report_path", C.c_char_p)]


class ScoreTableStruct(C.Structure):
    """bvcf_score_table"""
    _fields_ = [("entries", C.c_void_p), ("capacity", C.c_uint64), ("blob", C.c_void_p), ("blob_bytes", C.c_uint64),
                ("n", C.c_uint64), ("weights", C.c_void_p), ("n_columns", C.c_uint32), ("n_limbs", C.c_uint32),
                ("names", C.c_void_p), ("names_bytes", C.c_uint64)]


def score_weight(text):
    """bvcf_score_weight: a weight's text (bytes) -> the integer nearest to w 10^12, ties away from zero; ValueError for text
    that is no weight, OverflowError above 10^18  (host code, no device)"""
    out = C.c_int64(0)
    lib.bvcf_score_weight.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    rc = lib.bvcf_score_weight(bytes(text), len(text), C.byref(out))
    if rc == -2:
        raise OverflowError("weight above 10^6 in size")
    if rc:
        raise ValueError("not a weight")
    return int(out.value)


def score_limbs(w):
    """bvcf_score_limbs: W -> (its eight balanced base-256 digits, the smallest count that holds it)"""
    out = (C.c_int8 * 8)()
    lib.bvcf_score_limbs.argtypes = [C.c_int64, C.c_void_p]
    n = lib.bvcf_score_limbs(w, out)
    return [int(x) for x in out], int(n)


def score_decimal(t):
    """bvcf_score_decimal: the integer t (128 bits, two's complement) over 10^12 as exact decimal text"""
    v = t & ((1 << 128) - 1)
    out = C.create_string_buffer(48)
    lib.bvcf_score_decimal.restype = C.c_size_t
    lib.bvcf_score_decimal.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    n = lib.bvcf_score_decimal(v & ((1 << 64) - 1), v >> 64, out)
    return out.raw[:n]


class ScoreTable:
    """a host score table: bvcf_score_table_build over loci (bytes) and their integer weights W (a list of K per locus), or
    -- text= -- bvcf_score_table_parse over the bytes of a score file  (host code, no device)"""

    def __init__(self, loci=None, weights=None, names=None, text=None):
        self.t = ScoreTableStruct()
        if text is not None:
            err = C.create_string_buffer(512)
            lib.bvcf_score_table_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]
            rc = lib.bvcf_score_table_parse(bytes(text), len(text), C.byref(self.t), err, len(err))
            if rc:
                raise BvcfError(rc, err.value.decode())
            return
        loci = [bytes(x) for x in loci]
        w = np.ascontiguousarray(np.array(weights, dtype=np.int64).reshape(len(loci), -1) if len(loci) else
                                 np.zeros((0, len(names or [b"SCORE1"])), dtype=np.int64))
        k = w.shape[1]
        nm = b"".join(bytes(x) + b"\0" for x in (names or [b"SCORE%d" % (i + 1) for i in range(k)]))
        blob = b"".join(loci)
        lens = np.array([len(x) for x in loci], dtype=np.uint32)
        offs = np.zeros(len(loci), dtype=np.uint64)
        if len(loci) > 1:
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        lib.bvcf_score_table_build.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                               C.c_char_p, C.c_size_t, C.c_void_p]
        rc = lib.bvcf_score_table_build(blob, offs.ctypes.data if len(loci) else None, lens.ctypes.data if len(loci) else None,
                                        len(loci), w.ctypes.data if len(loci) else None, k, nm, len(nm), C.byref(self.t))
        if rc:
            raise BvcfError(rc, "bvcf_score_table_build")

    @property
    def n(self):
        return int(self.t.n)

    @property
    def capacity(self):
        return int(self.t.capacity)

    @property
    def n_columns(self):
        return int(self.t.n_columns)

    @property
    def n_limbs(self):
        return int(self.t.n_limbs)

    @property
    def names(self):
        return C.string_at(self.t.names, self.t.names_bytes).split(b"\0")[:-1] if self.t.names_bytes else []

    @property
    def weights(self):
        """the int8 weight rows [n][n_columns * n_limbs + 1] (copied)"""
        cols = self.n_columns * self.n_limbs + 1
        if not self.n:
            return np.zeros((0, cols), dtype=np.int8)
        return np.frombuffer(C.string_at(self.t.weights, self.n * cols), dtype=np.int8).reshape(self.n, cols).copy()

    @property
    def entries(self):
        """the slots as a VARIANT_ENTRY_DTYPE array (copied); the fourth word is the entry's weight row"""
        n = self.capacity * VARIANT_ENTRY_DTYPE.itemsize
        return np.frombuffer(C.string_at(self.t.entries, n), dtype=VARIANT_ENTRY_DTYPE).copy()

    def find(self, s):
        """bvcf_score_table_find: the entry's weight row by the probe the device runs, or -1"""
        lib.bvcf_score_table_find.restype = C.c_int64
        lib.bvcf_score_table_find.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        r = int(lib.bvcf_score_table_find(C.byref(self.t), bytes(s), len(s)))
        if r < -1:
            raise ValueError("bvcf_score_table_find: bad arguments")
        return r

    def close(self):
        lib.bvcf_score_table_free.argtypes = [C.c_void_p]
        lib.bvcf_score_table_free(C.byref(self.t))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CONFIG_MORE_ASSOC = 9  # BVCF_CONFIG_MORE_ASSOC in Config.reserved[1]: the ConfigScore is the head of a ConfigAssoc
ASSOC_ONE = 10 ** 6  # a phenotype's integer Y is in units of 10^-6
ASSOC_MAX_Y = 10 ** 12
ASSOC_MAX_COLUMNS = 16
ASSOC_COLUMNS = ["chrom", "pos", "ref", "alt", "pheno", "n", "altFreq", "beta", "se", "chisq", "p"]
ASSOC_REC_DTYPE = np.dtype([("n_het", "<u4"), ("n_hom", "<u4"), ("n_mis", "<u4"), ("pad", "<u4"), ("a_het", "<i8"), ("a_hom", "<i8"),
                            ("a_mis", "<i8"), ("b_mis_lo", "<u8"), ("b_mis_hi", "<u8")])  # bvcf_assoc_rec
PHENO_TOTALS_DTYPE = np.dtype([("np", "<u8"), ("ay", "<i8"), ("by_lo", "<u8"), ("by_hi", "<u8")])  # bvcf_pheno_totals


class ConfigAssoc(C.Structure):
    """bvcf_config_assoc: a bvcf_config_score and what came after it"""
    _fields_ = [("score", ConfigScore), ("pheno_path", C.c_char_p), ("assoc_path", C.c_char_p), ("assoc_report_path", C.c_char_p)]


class PhenoTableStruct(C.Structure):
    """bvcf_pheno_table"""
    _fields_ = [("n_columns", C.c_uint32), ("n_samples", C.c_uint32), ("s64", C.c_uint32), ("l1", C.c_uint32), ("l2", C.c_uint32),
                ("n_cols", C.c_uint32), ("n_named", C.c_uint64), ("b", C.c_void_p), ("y", C.c_void_p), ("present", C.c_void_p),
                ("totals", C.c_void_p), ("names", C.c_void_p), ("names_bytes", C.c_uint64)]


CONFIG_MORE_PCA = 10  # BVCF_CONFIG_MORE_PCA in Config.reserved[1]: the ConfigAssoc is the head of a ConfigPca
PCA_MAX_COMPONENTS = 64  # BVCF_PCA_MAX_COMPONENTS
PCA_DEFAULT_COMPONENTS = 10  # BVCF_PCA_DEFAULT_COMPONENTS


class ConfigPca(C.Structure):
    """bvcf_config_pca: a bvcf_config_assoc and what came after it"""
    _fields_ = [("assoc", ConfigAssoc), ("pca_prefix", C.c_char_p), ("pca_count", C.c_uint32), ("pca_reserved", C.c_uint32),
                ("pca_report_path", C.c_char_p)]


class AssocInfo(C.Structure):
    """bvcf_assoc_info"""
    _fields_ = [("recs", C.c_void_p), ("n_rows", C.c_uint64), ("need_rows", C.c_uint64), ("n_columns", C.c_uint32)]


CONFIG_MORE_COVAR = 11  # BVCF_CONFIG_MORE_COVAR in Config.reserved[1]: the ConfigPca is the head of a ConfigCovar
COVAR_MAX = 16  # BVCF_COVAR_MAX


class ConfigCovar(C.Structure):
    """bvcf_config_covar: a bvcf_config_pca and what came after it"""
    _fields_ = [("pca", ConfigPca), ("covar_path", C.c_char_p)]


class CovarTableStruct(C.Structure):
    """bvcf_covar_table"""
    _fields_ = [("n_covars", C.c_uint32), ("n_samples", C.c_uint32), ("s64", C.c_uint32), ("n_columns", C.c_uint32),
                ("n_groups", C.c_uint32), ("lc", C.c_uint32), ("lcc", C.c_uint32), ("lcy", C.c_uint32), ("n_blocks", C.c_uint32),
                ("row_words", C.c_uint32), ("n_named", C.c_uint64), ("n_incomplete", C.c_uint64), ("b", C.c_void_p), ("c", C.c_void_p),
                ("complete", C.c_void_p), ("group_of", C.c_void_p), ("group_first", C.c_void_p), ("pheno_np", C.c_void_p),
                ("totals", C.c_void_p), ("names", C.c_void_p), ("names_bytes", C.c_uint64)]


class AssocCovInfo(C.Structure):
    """bvcf_assoc_cov_info"""
    _fields_ = [("words", C.c_void_p), ("n_rows", C.c_uint64), ("row_words", C.c_uint32)]


CONFIG_MORE_LOGIT = 12  # BVCF_CONFIG_MORE_LOGIT in Config.reserved[1]: the ConfigCovar is the head of a ConfigLogit
ASSOC_MODELS = {"linear": 0, "logistic": 1}  # BVCF_ASSOC_MODEL_*
LOGIT_ONE = 1 << 24  # BVCF_LOGIT_ONE


class ConfigLogit(C.Structure):
    """bvcf_config_logit: a bvcf_config_covar and what came after it"""
    _fields_ = [("covar", ConfigCovar), ("assoc_model", C.c_uint32), ("reserved_logit", C.c_uint32)]


class LogitTableStruct(C.Structure):
    """bvcf_logit_table"""
    _fields_ = [("n_covars", C.c_uint32), ("n_samples", C.c_uint32), ("s64", C.c_uint32), ("n_columns", C.c_uint32),
                ("lwc", C.c_uint32), ("lr", C.c_uint32), ("lrc", C.c_uint32), ("lwcc", C.c_uint32), ("n_blocks", C.c_uint32),
                ("row_words", C.c_uint32), ("n_unfitted", C.c_uint32), ("pad", C.c_uint32), ("b", C.c_void_p), ("c", C.c_void_p),
                ("m", C.c_void_p), ("r", C.c_void_p), ("w", C.c_void_p), ("fitted", C.c_void_p), ("rounds", C.c_void_p),
                ("beta", C.c_void_p), ("pheno_np", C.c_void_p), ("totals", C.c_void_p)]


class AssocLogitInfo(C.Structure):
    """bvcf_assoc_logit_info"""
    _fields_ = [("words", C.c_void_p), ("n_rows", C.c_uint64), ("row_words", C.c_uint32)]


class PhenoTable:
    """a host phenotype table: bvcf_pheno_table_build over y / present (K lists of S integers Y and of S flags), or -- text=
    with sample_names= -- bvcf_pheno_table_parse over the bytes of a phenotype file  (host code, no device)"""

    def __init__(self, y=None, present=None, names=None, text=None, sample_names=None, n_named=0):
        self.t = PhenoTableStruct()
        if text is not None:
            sn = [bytes(x) for x in (sample_names or [])]
            ptrs = (C.c_char_p * max(len(sn), 1))(*sn)
            lens = (C.c_uint32 * max(len(sn), 1))(*[len(x) for x in sn])
            err = C.create_string_buffer(512)
            lib.bvcf_pheno_table_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.c_size_t]
            rc = lib.bvcf_pheno_table_parse(bytes(text), len(text), ptrs, lens, len(sn), C.byref(self.t), err, len(err))
            if rc:
                raise BvcfError(rc, err.value.decode(errors="replace"))
            return
        yy = np.ascontiguousarray(np.array(y, dtype=np.int64))
        k, s = yy.shape
        pp = np.ascontiguousarray(np.array(present, dtype=np.uint8).reshape(k, s))
        nm = b"".join(bytes(x) + b"\0" for x in (names or [b"PHENO%d" % (i + 1) for i in range(k)]))
        lib.bvcf_pheno_table_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t, C.c_uint64,
                                               C.c_void_p]
        rc = lib.bvcf_pheno_table_build(yy.ctypes.data if s else None, pp.ctypes.data if s else None, k, s, nm, len(nm), int(n_named),
                                        C.byref(self.t))
        if rc:
            raise BvcfError(rc, "bvcf_pheno_table_build")

    n_columns = property(lambda self: int(self.t.n_columns))
    n_samples = property(lambda self: int(self.t.n_samples))
    s64 = property(lambda self: int(self.t.s64))
    l1 = property(lambda self: int(self.t.l1))
    l2 = property(lambda self: int(self.t.l2))
    n_cols = property(lambda self: int(self.t.n_cols))
    n_named = property(lambda self: int(self.t.n_named))

    @property
    def names(self):
        return C.string_at(self.t.names, self.t.names_bytes).split(b"\0")[:-1] if self.t.names_bytes else []

    @property
    def b(self):
        """operand B, int8 [n_cols][s64] (copied)"""
        n = self.n_cols * self.s64
        return (np.frombuffer(C.string_at(self.t.b, n), dtype=np.int8).reshape(self.n_cols, self.s64).copy() if n else
                np.zeros((self.n_cols, 0), dtype=np.int8))

    @property
    def y(self):
        n = self.n_columns * self.n_samples
        return (np.frombuffer(C.string_at(self.t.y, 8 * n), dtype=np.int64).reshape(self.n_columns, self.n_samples).copy() if n else
                np.zeros((self.n_columns, 0), dtype=np.int64))

    @property
    def present(self):
        n = self.n_columns * self.n_samples
        return (np.frombuffer(C.string_at(self.t.present, n), dtype=np.uint8).reshape(self.n_columns, self.n_samples).copy() if n else
                np.zeros((self.n_columns, 0), dtype=np.uint8))

    @property
    def totals(self):
        """[(NP, AY, BY)] per column, Python integers"""
        t = np.frombuffer(C.string_at(self.t.totals, PHENO_TOTALS_DTYPE.itemsize * self.n_columns), dtype=PHENO_TOTALS_DTYPE)
        return [(int(x["np"]), int(x["ay"]), (int(x["by_hi"]) << 64) | int(x["by_lo"])) for x in t]

    def masked(self, complete):
        """bvcf_pheno_table_mask: a new PhenoTable with P = 0 wherever complete (S flags) is 0"""
        out = PhenoTable.__new__(PhenoTable)
        out.t = PhenoTableStruct()
        cp = np.ascontiguousarray(np.array(complete, dtype=np.uint8).reshape(self.n_samples))
        keep = cp if cp.size else np.zeros(1, dtype=np.uint8)
        lib.bvcf_pheno_table_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        rc = lib.bvcf_pheno_table_mask(C.byref(self.t), keep.ctypes.data, C.byref(out.t))
        if rc:
            raise BvcfError(rc, "bvcf_pheno_table_mask")
        return out

    def close(self):
        lib.bvcf_pheno_table_free.argtypes = [C.c_void_p]
        lib.bvcf_pheno_table_free(C.byref(self.t))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CovarTable:
    """a host covariate table: bvcf_covar_table_build over c / complete (J lists of S integers C and S flags), or -- text= with
    sample_names= -- bvcf_covar_table_parse over the bytes of a covariate file, which leaves an unbound table.  pheno= a MASKED
    PhenoTable (PhenoTable.masked(table.complete)) binds the table to it: groups, totals and operand B  (host code, no device)"""

    def __init__(self, c=None, complete=None, names=None, text=None, sample_names=None, n_named=0, pheno=None):
        self.t = CovarTableStruct()
        if text is not None:
            sn = [bytes(x) for x in (sample_names or [])]
            ptrs = (C.c_char_p * max(len(sn), 1))(*sn)
            lens = (C.c_uint32 * max(len(sn), 1))(*[len(x) for x in sn])
            err = C.create_string_buffer(512)
            lib.bvcf_covar_table_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.c_size_t]
            rc = lib.bvcf_covar_table_parse(bytes(text), len(text), ptrs, lens, len(sn), C.byref(self.t), err, len(err))
            if rc:
                raise BvcfError(rc, err.value.decode(errors="replace"))
            return
        cc = np.ascontiguousarray(np.array(c, dtype=np.int64))
        j, s = cc.shape
        cp = np.ascontiguousarray(np.array(complete, dtype=np.uint8).reshape(s))
        nm = b"".join(bytes(x) + b"\0" for x in (names or [b"COV%d" % (i + 1) for i in range(j)]))
        lib.bvcf_covar_table_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t, C.c_uint64,
                                               C.c_void_p, C.c_void_p]
        rc = lib.bvcf_covar_table_build(cc.ctypes.data if s else None, cp.ctypes.data if s else None, j, s, nm, len(nm), int(n_named),
                                        C.byref(pheno.t) if pheno is not None else None, C.byref(self.t))
        if rc:
            raise BvcfError(rc, "bvcf_covar_table_build")

    def bound(self, pheno):
        """the same covariates bound to a masked PhenoTable"""
        return CovarTable(self.c if self.n_samples else np.zeros((self.n_covars, 0), dtype=np.int64), self.complete, self.names,
                          n_named=self.n_named, pheno=pheno)

    n_covars = property(lambda self: int(self.t.n_covars))
    n_samples = property(lambda self: int(self.t.n_samples))
    s64 = property(lambda self: int(self.t.s64))
    n_columns = property(lambda self: int(self.t.n_columns))
    n_groups = property(lambda self: int(self.t.n_groups))
    lc = property(lambda self: int(self.t.lc))
    lcc = property(lambda self: int(self.t.lcc))
    lcy = property(lambda self: int(self.t.lcy))
    n_blocks = property(lambda self: int(self.t.n_blocks))
    row_words = property(lambda self: int(self.t.row_words))
    n_named = property(lambda self: int(self.t.n_named))
    n_incomplete = property(lambda self: int(self.t.n_incomplete))

    def _array(self, ptr, dtype, shape):
        n = int(np.prod(shape))
        if not n:
            return np.zeros(shape, dtype=dtype)
        return np.frombuffer(C.string_at(ptr, n * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()

    @property
    def names(self):
        return C.string_at(self.t.names, self.t.names_bytes).split(b"\0")[:-1] if self.t.names_bytes else []

    b = property(lambda self: self._array(self.t.b, np.int8, (16 * self.n_blocks, self.s64)))
    c = property(lambda self: self._array(self.t.c, np.int64, (self.n_covars, self.n_samples)))
    complete = property(lambda self: self._array(self.t.complete, np.uint8, (self.n_samples,)))
    group_of = property(lambda self: [int(x) for x in self._array(self.t.group_of, np.uint32, (self.n_columns,))])
    group_first = property(lambda self: [int(x) for x in self._array(self.t.group_first, np.uint32, (self.n_groups,))])
    totals = property(lambda self: self._array(self.t.totals, np.uint64, (self.row_words,)))

    def close(self):
        lib.bvcf_covar_table_free.argtypes = [C.c_void_p]
        lib.bvcf_covar_table_free(C.byref(self.t))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LogitTable:
    """bvcf_logit_table_build: the null fits, the fixed-point vectors M / R / W, the totals row and operand B from a PhenoTable
    (the masked one with covariates) and a CovarTable or None; BvcfError with the message for a value that is not 0 / 1
    (host code, no device)"""

    def __init__(self, pheno, covar=None):
        self.t = LogitTableStruct()
        err = C.create_string_buffer(512)
        lib.bvcf_logit_table_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        rc = lib.bvcf_logit_table_build(C.byref(pheno.t), C.byref(covar.t) if covar is not None else None, C.byref(self.t), err, len(err))
        if rc:
            raise BvcfError(rc, err.value.decode(errors="replace"))

    n_covars = property(lambda self: int(self.t.n_covars))
    n_samples = property(lambda self: int(self.t.n_samples))
    s64 = property(lambda self: int(self.t.s64))
    n_columns = property(lambda self: int(self.t.n_columns))
    lwc = property(lambda self: int(self.t.lwc))
    lr = property(lambda self: int(self.t.lr))
    lrc = property(lambda self: int(self.t.lrc))
    lwcc = property(lambda self: int(self.t.lwcc))
    n_blocks = property(lambda self: int(self.t.n_blocks))
    row_words = property(lambda self: int(self.t.row_words))
    n_unfitted = property(lambda self: int(self.t.n_unfitted))

    def _array(self, ptr, dtype, shape):
        n = int(np.prod(shape))
        if not n:
            return np.zeros(shape, dtype=dtype)
        return np.frombuffer(C.string_at(ptr, n * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()

    b = property(lambda self: self._array(self.t.b, np.int8, (16 * self.n_blocks, self.s64)))
    c = property(lambda self: self._array(self.t.c, np.int64, (self.n_covars, self.n_samples)))
    m = property(lambda self: self._array(self.t.m, np.int64, (self.n_columns, self.n_samples)))
    r = property(lambda self: self._array(self.t.r, np.int64, (self.n_columns, self.n_samples)))
    w = property(lambda self: self._array(self.t.w, np.int64, (self.n_columns, self.n_samples)))
    fitted = property(lambda self: [int(x) for x in self._array(self.t.fitted, np.uint8, (self.n_columns,))])
    rounds = property(lambda self: [int(x) for x in self._array(self.t.rounds, np.uint32, (self.n_columns,))])
    beta = property(lambda self: self._array(self.t.beta, np.float64, (self.n_columns, self.n_covars + 1)))
    totals = property(lambda self: self._array(self.t.totals, np.uint64, (self.row_words,)))

    def close(self):
        lib.bvcf_logit_table_free.argtypes = [C.c_void_p]
        lib.bvcf_logit_table_free(C.byref(self.t))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assoc_logit_stat(table, k, rec, totals, logit_row):
    """bvcf_assoc_logit_stat: phenotype k of a row from its record (as assoc_stat's), the phenotype's totals and the row's
    logistic record (row_words uint64) against a LogitTable -> (flags, [n, altFreq, beta, se, chisq, p]); flags bit 2:
    collinear  (host code, no device)"""
    r, t = _assoc_structs(rec, totals)
    w = np.ascontiguousarray(logit_row, dtype=np.uint64)
    assert w.size == table.row_words
    out = (C.c_double * 6)()
    lib.bvcf_assoc_logit_stat.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    flags = lib.bvcf_assoc_logit_stat(C.byref(table.t), int(k), r.ctypes.data, t.ctypes.data, w.ctypes.data, out)
    return int(flags), list(out)


def assoc_cov_stat(table, k, rec, totals, cov_row):
    """bvcf_assoc_cov_stat: phenotype k of a row from its record (as assoc_stat's), the phenotype's totals and the row's
    covariate record (row_words uint64) against a bound CovarTable -> (flags, [n, altFreq, beta, se, chisq, p]); flags bit 2:
    collinear  (host code, no device)"""
    r, t = _assoc_structs(rec, totals)
    w = np.ascontiguousarray(cov_row, dtype=np.uint64)
    assert w.size == table.row_words
    out = (C.c_double * 6)()
    lib.bvcf_assoc_cov_stat.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    flags = lib.bvcf_assoc_cov_stat(C.byref(table.t), int(k), r.ctypes.data, t.ctypes.data, w.ctypes.data, out)
    return int(flags), list(out)


def assoc_value(text):
    """bvcf_assoc_value: a value's text (bytes) -> the integer nearest to y 10^6, ties away from zero; ValueError for text that
    is no value, OverflowError above 10^6  (host code, no device)"""
    out = C.c_int64(0)
    lib.bvcf_assoc_value.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    rc = lib.bvcf_assoc_value(bytes(text), len(text), C.byref(out))
    if rc == -2:
        raise OverflowError("value above 10^6 in size")
    if rc:
        raise ValueError("not a value")
    return int(out.value)


def assoc_limbs(v):
    """bvcf_assoc_limbs: v (128 bits) -> (its sixteen balanced base-256 digits, the smallest count that holds it)"""
    out = (C.c_int8 * 16)()
    u = v & ((1 << 128) - 1)
    lib.bvcf_assoc_limbs.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    n = lib.bvcf_assoc_limbs(u & ((1 << 64) - 1), u >> 64, out)
    return [int(x) for x in out], int(n)


def _assoc_structs(rec, totals):
    r = np.zeros(1, dtype=ASSOC_REC_DTYPE)
    m64 = (1 << 64) - 1
    r[0] = (rec[0], rec[1], rec[2], 0, rec[3], rec[4], rec[5], rec[6] & m64, rec[6] >> 64)
    t = np.zeros(1, dtype=PHENO_TOTALS_DTYPE)
    t[0] = (totals[0], totals[1], totals[2] & m64, totals[2] >> 64)
    return r, t


def assoc_ints(rec, totals):
    """bvcf_assoc_ints: (n, Sg, c, va, vb) as Python integers, rec and totals as for assoc_stat"""
    r, t = _assoc_structs(rec, totals)
    out = (C.c_uint64 * 8)()
    lib.bvcf_assoc_ints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if lib.bvcf_assoc_ints(r.ctypes.data, t.ctypes.data, out):
        raise ValueError("bvcf_assoc_ints")
    def s64(x):
        return x - (1 << 64) if x >> 63 else x
    def s128(lo, hi):
        v = (hi << 64) | lo
        return v - (1 << 128) if v >> 127 else v
    return s64(out[0]), s64(out[1]), s128(out[2], out[3]), s128(out[4], out[5]), s128(out[6], out[7])


def assoc_stat(rec, totals):
    """bvcf_assoc_stat: rec = (n_het, n_hom, n_mis, a_het, a_hom, a_mis, b_mis), totals = (NP, AY, BY), Python integers ->
    (flags, [n, altFreq, beta, se, chisq, p])  (host code, no device)"""
    r, t = _assoc_structs(rec, totals)
    out = (C.c_double * 6)()
    lib.bvcf_assoc_stat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    flags = lib.bvcf_assoc_stat(r.ctypes.data, t.ctypes.data, out)
    return int(flags), list(out)


class RegionTableStruct(C.Structure):
    """bvcf_region_table"""
    _fields_ = [("chroms", C.c_void_p), ("capacity", C.c_uint64), ("blob", C.c_void_p), ("blob_bytes", C.c_uint64),
                ("intervals", C.c_void_p), ("n_intervals", C.c_uint64), ("n_chroms", C.c_uint64), ("n_keep", C.c_uint64),
                ("n_exclude", C.c_uint64), ("keep_given", C.c_uint32), ("max_name", C.c_uint32), ("raw", C.c_void_p)]


class RegionTable:
    """a host table of regions: SPEC lists (keep= / exclude=, bytes) and BED texts (keep_bed= / exclude_bed=, bytes) go
    through bvcf_region_table_parse_specs / _parse_bed, then bvcf_region_table_build.  A keep argument that is not None
    gives a keep set, even an empty one (b"" as keep_bed; an empty SPEC list is an error).  A parse error raises
    BvcfError with the library's message  (host code, no device)"""

    def __init__(self, keep=None, keep_bed=None, exclude=None, exclude_bed=None):
        self.t = RegionTableStruct()
        err = C.create_string_buffer(256)
        for fn in (lib.bvcf_region_table_parse_specs, lib.bvcf_region_table_parse_bed):
            fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
        for text, fn, excl in ((keep, lib.bvcf_region_table_parse_specs, 0), (keep_bed, lib.bvcf_region_table_parse_bed, 0),
                               (exclude, lib.bvcf_region_table_parse_specs, 1), (exclude_bed, lib.bvcf_region_table_parse_bed, 1)):
            if text is None:
                continue
            rc = fn(C.byref(self.t), bytes(text), len(text), excl, err, len(err))
            if rc:
                self.close()
                raise BvcfError(rc, err.value.decode(errors="replace"))
        lib.bvcf_region_table_build.argtypes = [C.c_void_p]
        rc = lib.bvcf_region_table_build(C.byref(self.t))
        if rc:
            self.close()
            raise BvcfError(rc, "bvcf_region_table_build")

    n_keep = property(lambda self: int(self.t.n_keep))
    n_exclude = property(lambda self: int(self.t.n_exclude))
    n_chroms = property(lambda self: int(self.t.n_chroms))
    capacity = property(lambda self: int(self.t.capacity))
    keep_given = property(lambda self: bool(self.t.keep_given))

    @property
    def blob(self):
        return C.string_at(self.t.blob, self.t.blob_bytes) if self.t.blob_bytes else b""

    @property
    def chroms(self):
        """the slots as a REGION_CHROM_DTYPE array (copied)"""
        n = self.capacity * REGION_CHROM_DTYPE.itemsize
        return np.frombuffer(C.string_at(self.t.chroms, n), dtype=REGION_CHROM_DTYPE).copy()

    @property
    def intervals(self):
        """all intervals as a REGION_INTERVAL_DTYPE array (copied); a name's are [first[s], first[s] + n[s])"""
        n = int(self.t.n_intervals) * REGION_INTERVAL_DTYPE.itemsize
        return np.frombuffer(C.string_at(self.t.intervals, n) if n else b"", dtype=REGION_INTERVAL_DTYPE).copy()

    def merged(self, exclude=False):
        """{normalised name: [(beg, end), ...]} of one set, as the table holds it"""
        iv, blob, s, out = self.intervals, self.blob, int(bool(exclude)), {}
        for c in self.chroms:
            if c["len"] and c["n"][s]:
                f = int(c["first"][s])
                out[blob[int(c["off"]):int(c["off"]) + int(c["len"])]] = [(int(x["beg"]), int(x["end"])) for x in iv[f:f + int(c["n"][s])]]
        return out

    def has(self, chrom, pos, alt):
        """bvcf_region_table_has: the lookup the device runs, for a row's TSV columns (bytes) -> bit 0: overlaps the keep
        set, bit 1: the exclude set"""
        lib.bvcf_region_table_has.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        r = lib.bvcf_region_table_has(C.byref(self.t), bytes(chrom), len(chrom), bytes(pos), len(pos), bytes(alt), len(alt))
        if r < 0:
            raise ValueError("bvcf_region_table_has: bad arguments")
        return int(r)

    def stays(self, chrom, pos, alt):
        """the rule of the flags on has()'s bits (bvcf_region_table_stays)"""
        lib.bvcf_region_table_stays.argtypes = [C.c_void_p, C.c_int]
        return bool(lib.bvcf_region_table_stays(C.byref(self.t), self.has(chrom, pos, alt)))

    def close(self):
        lib.bvcf_region_table_free.argtypes = [C.c_void_p]
        lib.bvcf_region_table_free(C.byref(self.t))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def region_gate_count(result):
    """bvcf_region_gate_count over a collected batch (a Result) -> [examined, kept, dropped]"""
    out = (C.c_uint64 * 3)()
    lib.bvcf_region_gate_count.restype = None
    lib.bvcf_region_gate_count.argtypes = [C.c_void_p, C.c_void_p]
    lib.bvcf_region_gate_count(C.byref(result), out)
    return [int(x) for x in out]


def variant_gate_count(result):
    """bvcf_variant_gate_count over a collected batch (a Result) -> [examined, kept, dropped]"""
    out = (C.c_uint64 * 3)()
    lib.bvcf_variant_gate_count.restype = None
    lib.bvcf_variant_gate_count.argtypes = [C.c_void_p, C.c_void_p]
    lib.bvcf_variant_gate_count(C.byref(result), out)
    return [int(x) for x in out]


class LdInfo(C.Structure):
    """bvcf_ld_info"""
    _fields_ = [("events", C.c_void_p), ("n_events", C.c_uint64), ("need_events", C.c_uint64), ("need_row_bytes", C.c_uint64),
                ("head_rows", C.c_void_p), ("tail_rows", C.c_void_p), ("n_rows", C.c_uint64), ("n_edge", C.c_uint32),
                ("row_bytes", C.c_uint32), ("window", C.c_uint32), ("reserved", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [
        ("batch_seq", C.c_uint64), ("status", C.c_int32), ("n_lines", C.c_uint32), ("n_alleles", C.c_uint32),
        ("n_errs", C.c_uint32), ("n_cmap_bytes", C.c_uint64), ("cmap_stride", C.c_uint32),
        ("n_samples", C.c_uint32), ("lines", C.c_void_p), ("alleles", C.c_void_p), ("errs", C.c_void_p),
        ("cmap", C.c_void_p), ("need_lines", C.c_uint64), ("need_alleles", C.c_uint64),
        ("need_cmap_bytes", C.c_uint64), ("kernel_ms", C.c_float), ("reserved", C.c_uint32),
        ("n_lines_seen", C.c_uint64), ("dosage", C.c_void_p), ("dosage_stride", C.c_uint32), ("reserved2", C.c_uint32),
        ("name_lists", C.c_void_p), ("names", C.c_void_p), ("n_name_bytes", C.c_uint64),
        ("text", C.c_void_p), ("n_text_bytes", C.c_uint64), ("head_off", C.c_void_p),
        ("sites", C.c_void_p), ("n_full_lines", C.c_uint32), ("n_row_cuts", C.c_uint32),
        ("rows", C.c_void_p), ("n_row_bytes", C.c_uint64), ("row_cuts", C.c_void_p), ("n_ok_sites", C.c_uint64),
    ]


ROW_CUT_DTYPE = np.dtype([("line", "<u4"), ("slot", "<u4"), ("off", "<u8"), ("text_off", "<u4"), ("reserved", "<u4")])
NO_TEXT_OFF = 0xFFFFFFFF
LINE_DTYPE = np.dtype([
    ("off", "<u4"), ("len", "<u4"), ("fend", "<u4", (9,)), ("rec_first", "<u4"), ("n_rec", "<u4"),
    ("n_fields", "<u4"), ("gt_task", "<u4"), ("status", "u1"), ("site_type", "u1"), ("pad", "u1", (2,))])
ALLELE_DTYPE = np.dtype([
    ("pos", "<i8"), ("line", "<u4"), ("alt_idx", "<u4"), ("alt_off", "<u4"), ("alt_len", "<u4"), ("ac", "<u4"),
    ("an", "<u4"), ("n_het", "<u4"), ("n_hom", "<u4"), ("n_miss", "<u4"), ("cmap_off", "<u4"), ("ref", "u1"),
    ("alt_base", "u1"), ("kind", "u1"), ("site_type", "u1"), ("trtv", "u1"), ("flags", "u1"), ("pad", "u1", (2,)),
    ("gt_task", "<u4"), ("pad2", "<u4")])
ERR_DTYPE = np.dtype([("line", "<u4"), ("alt_no", "<u4"), ("code", "<u4"), ("pad", "<u4")])
SITE_DTYPE = np.dtype([("off", "<u4"), ("len", "<u4"), ("fend", "u1", (8,)), ("ref", "u1"), ("alt_base", "u1"), ("trtv", "u1"),
                       ("status", "u1"), ("full_idx", "<u4"), ("n_fields", "<u4"), ("reserved", "<u4")])
SITE_FULL = 0x80
NAMES_DTYPE = np.dtype([("off", "<u4", (3,)), ("len", "<u4", (3,))])
assert LINE_DTYPE.itemsize == 64 and ALLELE_DTYPE.itemsize == 64 and ERR_DTYPE.itemsize == 16 and SITE_DTYPE.itemsize == 32

lib.bvcf_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Params)]
lib.bvcf_create.restype = C.c_int
lib.bvcf_destroy.argtypes = [C.c_void_p]
lib.bvcf_destroy.restype = None
lib.bvcf_last_error.argtypes = [C.c_void_p]
lib.bvcf_last_error.restype = C.c_char_p
lib.bvcf_version.restype = C.c_char_p
lib.bvcf_reserve.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
lib.bvcf_set_sample_names.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_char_p]
lib.bvcf_alloc_pinned.argtypes = [C.c_size_t]
lib.bvcf_alloc_pinned.restype = C.c_void_p
lib.bvcf_free_pinned.argtypes = [C.c_void_p]
lib.bvcf_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]
lib.bvcf_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]
lib.bvcf_submit_bgzf.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64]
lib.bvcf_collect.argtypes = [C.c_void_p, C.POINTER(Result)]
lib.bvcf_bench_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int,
                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
lib.bvcf_bench_device_slots.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int,
                                        C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
lib.bvcf_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
lib.bvcf_path.argtypes = [C.c_void_p]
lib.bvcf_sum_counters.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_uint64)]
lib.bvcf_allreduce_counters.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
lib.bvcf_device_count.restype = C.c_int
lib.bvcf_config_defaults.argtypes = [C.POINTER(Config)]
lib.bvcf_config_defaults.restype = None
lib.bvcf_string_header.argtypes = [C.POINTER(Config), C.c_char_p, C.c_size_t]
lib.bvcf_string_header.restype = C.c_size_t
lib.bvcf_format_tsv.argtypes = [C.POINTER(Config), C.POINTER(Result), C.c_void_p, C.POINTER(C.c_char_p),
                                C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
lib.bvcf_run_buffer.argtypes = [C.POINTER(Config), C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p),
                                C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                C.POINTER(C.c_uint64)]
lib.bvcf_run_fd.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
lib.bvcf_decompress_fd.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_char_p]
lib.bvcf_free.argtypes = [C.c_void_p]
lib.bvcf_free.restype = None


class RangePlan(C.Structure):
    _fields_ = [("data_off", C.c_uint64), ("range_bytes", C.c_uint64), ("spare_bytes", C.c_uint64), ("n_ranges", C.c_uint64)]


class TextCut(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_uint32), ("start", C.c_uint64), ("end", C.c_uint64), ("long_start", C.c_uint64)]


class ThreadBudget(C.Structure):
    _fields_ = [("readers", C.c_uint32), ("copy_threads", C.c_uint32), ("format_threads", C.c_uint32), ("busy_total", C.c_uint32)]


class PlanBlock(C.Structure):
    _fields_ = [("worker", C.c_uint32), ("piece", C.c_uint32), ("range", C.c_uint64), ("file_off", C.c_uint64),
                ("nbytes", C.c_uint64), ("own", C.c_uint64), ("first_off", C.c_uint32), ("bgzf", C.c_uint8),
                ("bgzf_flags", C.c_uint8), ("last_piece", C.c_uint8), ("reserved", C.c_uint8)]


CUT_LINES, CUT_NONE, CUT_LONG = 0, 1, 2
MODE_STREAM, MODE_TEXT_RANGES, MODE_BGZF_RANGES = 0, 1, 2
BGZF_SKIP_FIRST_LINE, BGZF_END_OF_STREAM = 1, 2
lib.bvcf_plan_text_ranges.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(RangePlan)]
lib.bvcf_plan_bgzf_ranges.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(RangePlan)]
lib.bvcf_cut_text_range.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint8, C.POINTER(TextCut)]
lib.bvcf_find_bgzf_chain.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t]
lib.bvcf_find_bgzf_chain.restype = C.c_long
lib.bvcf_plan_threads.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(ThreadBudget)]
lib.bvcf_plan_fd.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(PlanBlock), C.c_size_t,
                             C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(RangePlan)]


def plan_fd(fd_in, n_workers, max_batch_bytes=0, device_inflate=1, fd_err=2, cap=1 << 16):
    """the blocks bvcf_run_fd's readers would hand to n_workers device workers (no device involved)
    -> (rc, mode, RangePlan, [PlanBlock])"""
    out = (PlanBlock * cap)()
    n = C.c_size_t(0)
    mode = C.c_int(-1)
    plan = RangePlan()
    rc = lib.bvcf_plan_fd(fd_in, fd_err, n_workers, max_batch_bytes, device_inflate, out, cap, C.byref(n), C.byref(mode), C.byref(plan))
    assert n.value <= cap, "more blocks than room"
    return rc, mode.value, plan, [out[i] for i in range(n.value)]


HEAD_FAST_DECLINE, HEAD_FAST_PASS, HEAD_FAST_FILTER = 0, 1, 2
HAS_HEAD_BITS, NOT_REGULAR, DEFERRED = 0x80000000, 0x40000000, 0xFFFFFFFE


def head_fast_line(head, ls, len_flags, counts, cmap_off, tab_bits, line, n_header, allow="PASS,.", exclude=""):
    """k_order's fast lane on the host (include/bvcf_plan.h) -> (verdict, line record or None, allele record or None)"""
    # (bound here: BVCF_LIB may name an older build for an A/B run)
    lib.bvcf_head_fast_line.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                        C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]
    L = np.zeros(1, dtype=LINE_DTYPE)
    A = np.zeros(1, dtype=ALLELE_DTYPE)
    v = lib.bvcf_head_fast_line(bytes(head), len(head), ls, len_flags, (C.c_uint32 * 5)(*counts), cmap_off,
                                (C.c_uint32 * 8)(*tab_bits), line, n_header, allow.encode(), exclude.encode(),
                                L.ctypes.data, A.ctypes.data)
    return v, (L[0] if v != HEAD_FAST_DECLINE else None), (A[0] if v == HEAD_FAST_PASS else None)


CHAIN_STREAM, CHAIN_SITES2_TILES, CHAIN_SITES2_CHUNKS, CHAIN_CENSUS, CHAIN_SITES_EXP, CHAIN_SITES1_EXP = range(6)
SCAN_NONE, SCAN_PLAIN, SCAN_WIDE, SCAN_FILTER, SCAN_SUBSET = range(5)
WIDE_SAMPLES = 32768  # BVCF_WIDE_SAMPLES


class CtxPlan(C.Structure):
    """bvcf_ctx_plan (include/bvcf_plan.h): what bvcf_create decides before it touches the device"""
    _fields_ = [("max_batch_bytes", C.c_uint64), ("max_lines", C.c_uint64), ("max_alleles", C.c_uint64), ("max_cmap", C.c_uint64),
                ("n_slots", C.c_uint32), ("n_samples", C.c_uint32), ("n_samples_full", C.c_uint32), ("cmap_stride", C.c_uint32),
                ("dosage_stride", C.c_uint32), ("tile_bytes", C.c_uint32), ("tile_quota", C.c_uint32), ("win_bytes", C.c_uint32),
                ("chain", C.c_uint32), ("scan", C.c_uint32), ("gen_policy", C.c_int32), ("ss_ns_pad", C.c_uint32),
                ("ss_max_runs", C.c_uint32), ("ss_stripes", C.c_uint32), ("s1_fmode", C.c_uint32), ("s1_fkey", C.c_uint32 * 4),
                ("s1_flen", C.c_uint32 * 4), ("eol_byte", C.c_uint8), ("packed", C.c_uint8), ("render", C.c_uint8),
                ("gen_mode", C.c_uint8), ("shape_seen", C.c_uint8), ("head_fast", C.c_uint8), ("ss_on", C.c_uint8),
                ("reserved", C.c_uint8)]


def make_params(n_header_fields, allow="PASS,.", exclude="", device=0, eol_chars=1, eol_byte=b"\n", max_batch_bytes=0,
                max_lines=0, max_alleles=0, cmap_bytes=0, n_slots=0, want_class_maps=True, path=0, want_dosage=False,
                want_name_lists=False, packed_sites=False, render_sites=False, sample_stats=False, min_gq=0, min_dp=0,
                sample_keep=None):
    """bvcf_params as Ctx fills them (sample_keep: the indices of the kept samples); keeps its strings and mask alive"""
    p = Params()
    p.abi_version = ABI_VERSION
    p.device = device
    p.n_header_fields = n_header_fields
    p.eol_chars = eol_chars
    p.eol_byte = eol_byte[0]
    p.want_class_maps = int(want_class_maps)
    p.want_dosage = int(want_dosage)
    p._keep = [allow.encode(), exclude.encode()]
    p.allow_filter, p.exclude_filter = p._keep
    p.max_batch_bytes = max_batch_bytes
    p.max_lines = max_lines
    p.max_alleles = max_alleles
    p.cmap_bytes = cmap_bytes
    p.n_slots = n_slots
    p.path = path
    p.packed_sites = int(packed_sites or render_sites)
    p.render_sites = int(render_sites)
    p.want_name_lists = int(want_name_lists)
    p.want_sample_stats = int(sample_stats)
    p.min_gq = min_gq  # bvcf_params.min_gq / min_dp: the masked genotype scan (0 = off)
    p.min_dp = min_dp
    if sample_keep is not None:
        # bvcf_params.sample_keep: everything the ctx returns is then indexed by a sample's rank among the kept ones
        words = (C.c_uint32 * max((max(n_header_fields - 9, 0) + 31) // 32, 1))()
        for s in set(int(s) for s in sample_keep):
            if 0 <= s < 32 * len(words):  # (bits at or beyond n_samples are the library's to ignore)
                words[s >> 5] |= 1 << (s & 31)
        p.abi_version = ABI_VERSION_SUBSET
        p.sample_keep = words  # (bvcf_create copies it)
    return p


def plan_ctx(n_header_fields, **params):
    """the plan of a ctx with these make_params arguments, made without a device -> (rc, CtxPlan)"""
    lib.bvcf_plan_ctx.argtypes = [C.POINTER(Params), C.POINTER(CtxPlan)]  # (bound here: BVCF_LIB may name an older build)
    p = make_params(n_header_fields, **params)
    out = CtxPlan()
    return lib.bvcf_plan_ctx(C.byref(p), C.byref(out)), out


class BvcfError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__("bvcf error %d: %s" % (rc, msg))
        self.rc = rc


def make_config(cfg=None, device=0, max_batch_bytes=0, n_format_threads=0):
    """cfg uses the key names of tests/golden/known_answers.json (emptyField, keepId, allow, ...).
    The returned object keeps the byte strings alive."""
    cfg = cfg or {}
    # (--mendel / --mendelErrors: the larger struct and its marker, only then; every other config is a ConfigMore as before)
    # (--ld / --ldPrune: the still larger struct and its marker, only then)
    # (--keepVariants / --excludeVariants / --variantFilterReport: the largest struct and its marker, only then)
    # (--regions / --excludeRegions, their files, --regionFilterReport: the struct behind that one and its marker, only then)
    # (--grm: the struct behind that one and its marker, only then)
    # (--score / --scoreOutput / --scoreReport: the struct behind that one and its marker, only then)
    # (--pheno / --assoc / --assocReport: the struct behind that one and its marker, only then)
    # (--pca / --pcaCount / --pcaReport: the struct behind that one and its marker, only then)
    # (--covar: the struct behind that one and its marker, only then)
    # (--assocModel: the struct behind that one and its marker, only then)
    lgc = ConfigLogit() if cfg.get("assocModel") is not None else None
    cvc = lgc.covar if lgc is not None else ConfigCovar() if cfg.get("covar") else None
    pc = cvc.pca if cvc is not None else ConfigPca() if any(cfg.get(k) for k in ("pca", "pcaCount", "pcaReport")) else None
    ac = pc.assoc if pc is not None else ConfigAssoc() if any(cfg.get(k) for k in ("pheno", "assoc", "assocReport")) else None
    sc = ac.score if ac is not None else ConfigScore() if any(cfg.get(k) for k in ("score", "scoreOutput", "scoreReport")) else None
    gc = sc.grm if sc is not None else ConfigGrm() if cfg.get("grm") else None
    rgc = gc.regions if gc is not None else ConfigRegions() if any(cfg.get(k) for k, _ in REGION_CONFIG_KEYS) else None
    vc = (rgc.variants if rgc is not None else
          ConfigVariants() if any(cfg.get(k) for k in ("keepVariants", "excludeVariants", "variantFilterReport")) else None)
    ldc = vc.ld if vc is not None else ConfigLd() if cfg.get("ld") or cfg.get("ldPrune") else None
    trios = ldc.trios if ldc is not None else ConfigTrios() if cfg.get("mendel") or cfg.get("mendelErrors") else None
    more = trios.more if trios is not None else ConfigMore()
    c = more.base  # (a view of more's memory, which it keeps alive: what the callers pass on is the head of a bvcf_config_more)
    lib.bvcf_config_defaults(C.byref(c))
    keep = [cfg.get("emptyField", "!").encode(), cfg.get("fieldDelimiter", ";").encode(),
            cfg.get("allow", "PASS,.").encode(), cfg.get("exclude", "").encode()]
    c.empty_field, c.field_delimiter, c.allow_filter, c.exclude_filter = keep
    c.keep_id = int(cfg.get("keepId", False))
    c.keep_info = int(cfg.get("keepInfo", False))
    c.keep_pos = int(cfg.get("keepPos", False))
    c.normalize_header = int(cfg.get("normalizeHeader", True))
    c.device = device
    c.max_batch_bytes = max_batch_bytes
    c.n_format_threads = n_format_threads
    if cfg.get("sample"):
        keep.append(cfg["sample"].encode())
        c.sample_list_path = keep[-1]
    if cfg.get("dosageOutput"):
        keep.append(str(cfg["dosageOutput"]).encode())
        c.dosage_path = keep[-1]
    c.no_out = int(cfg.get("noOut", False))
    c.out_bgzf = int(cfg.get("compressOutput", "none") == "bgzf")  # bvcf_run_fd only
    if cfg.get("devices"):  # bvcf_run_fd only: the device list the blocks are dealt to
        arr = (C.c_int32 * len(cfg["devices"]))(*cfg["devices"])
        keep.append(arr)
        c.devices = arr
        c.n_devices = len(cfg["devices"])
    if cfg.get("sampleStats"):  # the per-sample QC table of the run (SAMPLE_STATS_COLUMNS)
        keep.append(str(cfg["sampleStats"]).encode())
        c.sample_stats_path = keep[-1]
    # --minGQ / --minDP: genotypes whose GQ / DP is a number below the threshold count as missing (0 = off)
    c.min_gq = int(cfg.get("minGQ", 0))
    c.min_dp = int(cfg.get("minDP", 0))
    # --keepSamples / --excludeSamples: the path of a list of sample names; the run works on those / on all but those
    if cfg.get("keepSamples"):
        keep.append(str(cfg["keepSamples"]).encode())
        c.keep_samples_path = keep[-1]
    if cfg.get("excludeSamples"):
        keep.append(str(cfg["excludeSamples"]).encode())
        c.exclude_samples_path = keep[-1]
    if cfg.get("relatedness"):  # the pairwise table of the run (PAIR_STATS_COLUMNS)
        keep.append(str(cfg["relatedness"]).encode())
        more.pair_stats_path = keep[-1]
        c.reserved[0] = CONFIG_MORE
    # --minMaf / --maxMaf / --minMac / --maxMissing / --hwe: the site gate of the run; --siteFilterReport: its counts
    if any(k in cfg for k in GATE_KEYS) or cfg.get("siteFilterReport"):
        more.site_gate = make_site_gate(**{k: cfg[k] for k in GATE_KEYS if k in cfg})
        if cfg.get("siteFilterReport"):
            keep.append(str(cfg["siteFilterReport"]).encode())
            more.site_filter_path = keep[-1]
        c.reserved[0] = CONFIG_MORE
        c.reserved[1] = CONFIG_MORE_GATE
    if cfg.get("plinkOutput"):  # PREFIX.bed / .bim / .fam of the run's rows (the third marker implies the gate fields)
        if not c.reserved[1]:
            more.site_gate = make_site_gate()
        keep.append(str(cfg["plinkOutput"]).encode())
        more.plink_prefix = keep[-1]
        c.reserved[0] = CONFIG_MORE
        c.reserved[1] = CONFIG_MORE_PLINK
    if trios is not None:  # the pedigree and the two tables (the fourth marker implies the gate fields and the prefix)
        if not c.reserved[1]:
            more.site_gate = make_site_gate()
        for key, field in (("fam", "fam_path"), ("mendel", "mendel_path"), ("mendelErrors", "mendel_errors_path")):
            if cfg.get(key):
                keep.append(str(cfg[key]).encode())
                setattr(trios, field, keep[-1])
        c.reserved[0] = CONFIG_MORE
        c.reserved[1] = CONFIG_MORE_TRIOS
    if ldc is not None:  # the table, the prune prefix, the window and the threshold (ldR2: the flag's text)
        for key, field in (("ld", "ld_path"), ("ldPrune", "ld_prune_prefix")):
            if cfg.get(key):
                keep.append(str(cfg[key]).encode())
                setattr(ldc, field, keep[-1])
        ldc.ld_window = int(cfg.get("ldWindow", 50))
        ldc.ld_t6 = parse_ld_r2(str(cfg.get("ldR2", "0.2")))
        ldc.ld_t6_set = 1
        c.reserved[1] = CONFIG_MORE_LD
    if vc is not None:  # the list of locus strings and its report
        for key, field in (("keepVariants", "keep_variants_path"), ("excludeVariants", "exclude_variants_path"),
                           ("variantFilterReport", "variant_filter_path")):
            if cfg.get(key):
                keep.append(str(cfg[key]).encode())
                setattr(vc, field, keep[-1])
        c.reserved[1] = CONFIG_MORE_VARIANTS
    if rgc is not None:  # the regions and their report
        for key, field in REGION_CONFIG_KEYS:
            if cfg.get(key):
                keep.append(str(cfg[key]).encode())
                setattr(rgc, field, keep[-1])
        c.reserved[1] = CONFIG_MORE_REGIONS
    if gc is not None:  # PREFIX.grm.bin / .grm.N.bin / .grm.id of the run's rows
        if cfg.get("grm"):
            keep.append(str(cfg["grm"]).encode())
            gc.grm_prefix = keep[-1]
        c.reserved[1] = CONFIG_MORE_GRM
    if sc is not None:  # the score file, the table of per-sample scores and the report
        for key, field in (("score", "score_path"), ("scoreOutput", "score_output_path"), ("scoreReport", "score_report_path")):
            if cfg.get(key):
                keep.append(str(cfg[key]).encode())
                setattr(sc, field, keep[-1])
        c.reserved[1] = CONFIG_MORE_SCORE
    if ac is not None:  # the phenotype file, the scan's table and the report
        for key, field in (("pheno", "pheno_path"), ("assoc", "assoc_path"), ("assocReport", "assoc_report_path")):
            if cfg.get(key):
                keep.append(str(cfg[key]).encode())
                setattr(ac, field, keep[-1])
        c.reserved[1] = CONFIG_MORE_ASSOC
    if pc is not None:  # PREFIX.eigenvec / .eigenval of the run's relationship matrix, how many components, the report
        for key, field in (("pca", "pca_prefix"), ("pcaReport", "pca_report_path")):
            if cfg.get(key):
                keep.append(str(cfg[key]).encode())
                setattr(pc, field, keep[-1])
        pc.pca_count = int(cfg.get("pcaCount") or PCA_DEFAULT_COMPONENTS)
        c.reserved[1] = CONFIG_MORE_PCA
    if cvc is not None:  # the covariate file of the scan
        if cfg.get("covar"):
            keep.append(str(cfg["covar"]).encode())
            cvc.covar_path = keep[-1]
        c.reserved[1] = CONFIG_MORE_COVAR
    if lgc is not None:  # the scan's model: "linear" / "logistic", or the number itself
        m = cfg["assocModel"]
        lgc.assoc_model = ASSOC_MODELS[m] if m in ASSOC_MODELS else int(m)
        c.reserved[1] = CONFIG_MORE_LOGIT
    c._keep = keep
    return c


def grm_matrix(tables, n_samples):
    """bvcf_grm_matrix: the uint64 words bvcf_grm gives (3 S S + 1 of them) -> (lower, counts), the float32 lower triangles
    of PREFIX.grm.bin and PREFIX.grm.N.bin  (host code, no device)"""
    t = np.ascontiguousarray(tables, dtype=np.uint64).ravel()
    s = int(n_samples)
    assert t.size == 3 * s * s + 1
    lower = np.zeros(s * (s + 1) // 2, dtype=np.float32)
    counts = np.zeros(s * (s + 1) // 2, dtype=np.float32)
    lib.bvcf_grm_matrix.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    rc = lib.bvcf_grm_matrix(t.ctypes.data, s, lower.ctypes.data, counts.ctypes.data)
    if rc:
        raise BvcfError(rc, "bvcf_grm_matrix")
    return lower, counts


def pca_tridiag(d, e, k):
    """bvcf_pca_tridiag: the k largest eigenvalues, descending, of the symmetric tridiagonal matrix (d, e) and a unit vector
    for each -> (values (k,), vectors (k, n))  (host code, no device)"""
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    n = d.size
    assert e.size == max(n - 1, 0)
    values = np.zeros(max(int(k), 0), dtype=np.float64)
    z = np.zeros((max(int(k), 0), n), dtype=np.float64)
    lib.bvcf_pca_tridiag.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    rc = lib.bvcf_pca_tridiag(d.ctypes.data, e.ctypes.data if e.size else None, n, int(k), values.ctypes.data, z.ctypes.data)
    if rc:
        raise BvcfError(rc, "bvcf_pca_tridiag")
    return values, z


def pca_eigen(lower, n_samples, k, device=0, timings=None):
    """bvcf_pca_eigen: the packed float32 lower triangle of a symmetric matrix (S (S + 1) / 2 values, row by row) -> (values (k,),
    vectors (k, S)): the k largest eigenvalues, descending, and unit eigenvectors, largest component positive.  timings: a
    list that receives the five phase times in ms (bvcf_bench_pca_eigen)"""
    a = np.ascontiguousarray(lower, dtype=np.float32).ravel()
    s, k = int(n_samples), int(k)
    assert a.size == s * (s + 1) // 2
    values = np.zeros(max(k, 0), dtype=np.float64)
    vectors = np.zeros((max(k, 0), s), dtype=np.float64)
    if timings is not None:
        ms = (C.c_float * 5)()
        lib.bvcf_bench_pca_eigen.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        rc, msg = lib.bvcf_bench_pca_eigen(device, a.ctypes.data, s, k, values.ctypes.data, vectors.ctypes.data, ms), "bvcf_bench_pca_eigen"
        timings[:] = list(ms)
    else:
        err = C.create_string_buffer(256)
        lib.bvcf_pca_eigen.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        rc = lib.bvcf_pca_eigen(device, a.ctypes.data, s, k, values.ctypes.data, vectors.ctypes.data, err, len(err))
        msg = err.value.decode()
    if rc:
        raise BvcfError(rc, msg)
    return values, vectors


def ld_counts(row_a, row_b, n_samples):
    """bvcf_ld_counts: two rows in .bed code (bytes-like, ceil(S / 4) bytes) -> [n, sa, sb, saa, sbb, sab]  (host code, no device)"""
    rb = (n_samples + 3) // 4
    a = (C.c_uint8 * rb).from_buffer_copy(bytes(row_a)[:rb])
    b = (C.c_uint8 * rb).from_buffer_copy(bytes(row_b)[:rb])
    out = (C.c_uint32 * 6)()
    lib.bvcf_ld_counts.restype = C.c_int
    lib.bvcf_ld_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    if lib.bvcf_ld_counts(a, b, n_samples, out):
        raise ValueError("bvcf_ld_counts: bad arguments")
    return [int(x) for x in out]


def ld_in_ld(counts, t6):
    """bvcf_ld_in_ld: the exact 128-bit predicate on [n, sa, sb, saa, sbb, sab] at t6 millionths -> bool  (host code)"""
    k = (C.c_uint32 * 6)(*[int(x) for x in counts])
    lib.bvcf_ld_in_ld.restype = C.c_int
    lib.bvcf_ld_in_ld.argtypes = [C.c_void_p, C.c_uint32]
    r = lib.bvcf_ld_in_ld(k, t6)
    if r < 0:
        raise ValueError("bvcf_ld_in_ld: bad arguments")
    return bool(r)


def parse_ld_r2(text):
    """bvcf_parse_ld_r2: the text of --ldR2 -> millionths; ValueError for a text outside the flag's rules"""
    t6 = C.c_uint32()
    lib.bvcf_parse_ld_r2.restype = C.c_int
    lib.bvcf_parse_ld_r2.argtypes = [C.c_char_p, C.c_void_p]
    if lib.bvcf_parse_ld_r2(text.encode() if isinstance(text, str) else bytes(text), C.byref(t6)):
        raise ValueError("ldR2: %r" % (text,))
    return int(t6.value)


class LdSeam:
    """bvcf_ld_seam_*: the state machine behind --ld / --ldPrune, fed batches cut anywhere (host code, no device)"""

    def __init__(self, n_samples, window, t6):
        lib.bvcf_ld_seam_create.restype = C.c_void_p
        lib.bvcf_ld_seam_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        self.h = lib.bvcf_ld_seam_create(n_samples, window, t6)
        if not self.h:
            raise ValueError("bvcf_ld_seam_create: bad arguments")
        self.window, self.rb = window, (n_samples + 3) // 4

    def push(self, rows, events, loci):
        """rows: uint8 (n_rows, row_bytes) in .bed code -- only the first and last min(window, n_rows) are handed on, as a
        ctx gives them; events: uint32 (n, 8), rows local to the batch; loci: list of bytes "chrom\tpos\tref\talt" """
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(len(loci), self.rb)
        n = len(loci)
        k = min(self.window, n)
        head, tail = np.ascontiguousarray(rows[:k]), np.ascontiguousarray(rows[n - k:])
        return self.push_edges(n, head, tail, events, loci)

    def push_edges(self, n_rows, head, tail, events, loci):
        ev = np.ascontiguousarray(events, dtype=np.uint32).reshape(-1, 8)
        text = b"".join(loci)
        off = np.zeros(n_rows + 1, dtype=np.uint64)
        if n_rows:
            off[1:] = np.cumsum([len(x) for x in loci])
        head = np.ascontiguousarray(head, dtype=np.uint8)
        tail = np.ascontiguousarray(tail, dtype=np.uint8)
        buf = C.create_string_buffer(text, len(text) + 1)
        lib.bvcf_ld_seam_push.restype = C.c_int
        lib.bvcf_ld_seam_push.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.c_void_p, C.c_void_p]
        rc = lib.bvcf_ld_seam_push(self.h, n_rows, min(self.window, n_rows), head.ctypes.data if head.size else None,
                                   tail.ctypes.data if tail.size else None, ev.ctypes.data if len(ev) else None, len(ev), buf,
                                   off.ctypes.data)
        if rc:
            raise ValueError("bvcf_ld_seam_push: the batch contradicts itself")

    def read(self, which):
        """0: the table's lines (no header), 1: .prune.in, 2: .prune.out -> bytes"""
        p, n = C.c_void_p(), C.c_size_t()
        lib.bvcf_ld_seam_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        if lib.bvcf_ld_seam_read(self.h, which, C.byref(p), C.byref(n)):
            raise ValueError("bvcf_ld_seam_read")
        return C.string_at(p.value, n.value) if n.value else b""

    def counts(self):
        lib.bvcf_ld_seam_rows.restype = lib.bvcf_ld_seam_pairs.restype = C.c_uint64
        lib.bvcf_ld_seam_rows.argtypes = lib.bvcf_ld_seam_pairs.argtypes = [C.c_void_p]
        return int(lib.bvcf_ld_seam_rows(self.h)), int(lib.bvcf_ld_seam_pairs(self.h))

    def close(self):
        if self.h:
            lib.bvcf_ld_seam_destroy.argtypes = [C.c_void_p]
            lib.bvcf_ld_seam_destroy(self.h)
            self.h = None

    __del__ = close


def trio_verdict(child, father, mother):
    """bvcf_trio_verdict: TRIO_* for the classes (none 0, het 1, hom 2, missing 3) of a trio in a row (host code, no device)"""
    lib.bvcf_trio_verdict.restype = C.c_int
    lib.bvcf_trio_verdict.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    return lib.bvcf_trio_verdict(child, father, mother)


def parse_fam(text, names):
    """bvcf_parse_fam: a PLINK .fam (bytes) against the sample names (list of bytes, header order) -> (FAM_OK, [(child,
    father, mother), ...] by child) or (FAM_* reason, 1-based line, the line's IID or None)  (host code, no device)"""
    n = len(names)
    arr = (C.c_char_p * max(n, 1))(*names)
    lens = (C.c_uint32 * max(n, 1))(*[len(x) for x in names])
    out = (C.c_uint32 * (3 * max(n, 1)))()
    n_trios, bad_line, iid, iid_len = C.c_size_t(), C.c_uint64(), C.c_void_p(), C.c_size_t()
    buf = C.create_string_buffer(bytes(text), len(text) + 1)
    lib.bvcf_parse_fam.restype = C.c_int
    lib.bvcf_parse_fam.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    why = lib.bvcf_parse_fam(buf, len(text), arr, lens, n, out, n, C.byref(n_trios), C.byref(bad_line), C.byref(iid),
                             C.byref(iid_len))
    if why:
        return why, int(bad_line.value), (C.string_at(iid.value, iid_len.value) if iid.value else None)
    return FAM_OK, [tuple(out[3 * t:3 * t + 3]) for t in range(n_trios.value)]


def bed_row(cmap, n_samples, sparse=False, out=None):
    """bvcf_bed_row: one class map -- dense, padded to 16 bytes as the library lays it out, or a short list (uint32 n, then
    n entries) -- into the ceil(S / 4) bytes of its .bed row (host code, no device).  out: a uint8 array to write into at
    offset 0 (the return value is then the length); otherwise the row is returned as bytes.  cmap None: a record without a
    map"""
    rb = (n_samples + 3) // 4
    buf = out if out is not None else np.zeros(rb, dtype=np.uint8)
    src = None if cmap is None else np.ascontiguousarray(np.frombuffer(bytes(cmap), dtype=np.uint8))
    lib.bvcf_bed_row.restype = C.c_int
    lib.bvcf_bed_row.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
    n = lib.bvcf_bed_row(None if src is None else src.ctypes.data, int(sparse), n_samples, buf.ctypes.data)
    if n != rb:
        raise BvcfError(E_ARG, "bvcf_bed_row")
    return n if out is not None else buf.tobytes()


def hwe_exact(het, hom, other):
    """bvcf_hwe_exact: the exact Hardy-Weinberg p value as the site gate defines it (host code, no device)"""
    lib.bvcf_hwe_exact.restype = C.c_double
    lib.bvcf_hwe_exact.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    return lib.bvcf_hwe_exact(het, hom, other)


def hwe_inline_terms():
    """bvcf_hwe_inline_terms: supports of the exact test up to this many terms are summed by one thread of k_site_gate,
    longer ones by a wave of k_site_hwe"""
    lib.bvcf_hwe_inline_terms.restype = C.c_uint32
    lib.bvcf_hwe_inline_terms.argtypes = []
    return lib.bvcf_hwe_inline_terms()


def site_gate_verdict(gate, n_samples, counts):
    """bvcf_site_gate_verdict: the GATE_* bits an examined row fails; gate: a SiteGate or make_site_gate's keywords as a
    dict; counts = (ac, an, n_het, n_hom, n_miss) (host code, no device)"""
    g = gate if isinstance(gate, SiteGate) else make_site_gate(**gate)
    arr = (C.c_uint32 * 5)(*[int(x) for x in counts])
    lib.bvcf_site_gate_verdict.restype = C.c_int
    lib.bvcf_site_gate_verdict.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return lib.bvcf_site_gate_verdict(C.byref(g), n_samples, arr)


def site_gate_count(result):
    """bvcf_site_gate_count over a collected batch (a Result, or a Batch's .r) -> the seven counts of SITE_GATE_REPORT"""
    out = (C.c_uint64 * 7)()
    lib.bvcf_site_gate_count.restype = None
    lib.bvcf_site_gate_count.argtypes = [C.c_void_p, C.c_void_p]
    lib.bvcf_site_gate_count(C.byref(result), out)
    return list(out)


def bench_hwe(triples, device=0):
    """bvcf_bench_hwe: the device's exact test on each (het, hom, other) -> float64 array"""
    t = np.ascontiguousarray(np.asarray(triples, dtype=np.uint32).reshape(-1, 3))
    p = np.zeros(len(t), dtype=np.float64)
    lib.bvcf_bench_hwe.restype = C.c_int
    lib.bvcf_bench_hwe.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    rc = lib.bvcf_bench_hwe(device, t.ctypes.data, len(t), p.ctypes.data)
    if rc:
        raise BvcfError(rc, "bvcf_bench_hwe")
    return p


def bench_deflate_codes(cases, device=0):
    """bvcf_bench_deflate_codes: step 4 of k_deflate on each (hll[286], hd[30], text bytes) ->
    (lens uint8 [n, 335] = 286 + 30 + 19 code lengths, rle uint16 [n, 316] = symbol | extra << 8,
     out uint32 [n, 8] = kind, header bits, hlit, hdist, hclen, entries, dyn_bytes, fix_bytes)"""
    hist = np.zeros((len(cases), 317), dtype=np.uint32)
    for i, (hll, hd, n) in enumerate(cases):
        hist[i, :286], hist[i, 286:316], hist[i, 316] = hll, hd, n
    lens = np.zeros((len(cases), 335), dtype=np.uint8)
    rle = np.zeros((len(cases), 316), dtype=np.uint16)
    out = np.zeros((len(cases), 8), dtype=np.uint32)
    lib.bvcf_bench_deflate_codes.restype = C.c_int
    lib.bvcf_bench_deflate_codes.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = lib.bvcf_bench_deflate_codes(device, hist.ctypes.data, len(cases), lens.ctypes.data, rle.ctypes.data, out.ctypes.data)
    if rc:
        raise BvcfError(rc, "bvcf_bench_deflate_codes")
    return lens, rle, out


def guard_check():
    """bvcf_bench_guard_check (BVCF_POISON, tests only): the guard zones around every live device and pinned buffer, and
    what the freed ones recorded -> (buffers damaged since the last call, the report of the first one or "")"""
    msg = C.create_string_buffer(256)
    lib.bvcf_bench_guard_check.restype = C.c_ulong
    lib.bvcf_bench_guard_check.argtypes = [C.c_char_p, C.c_size_t]
    n = lib.bvcf_bench_guard_check(msg, len(msg))
    return int(n), msg.value.decode(errors="replace")


def guarded_buffers():
    """bvcf_bench_guarded_buffers: the buffers BVCF_POISON holds between guards at the moment (0 when the mode is off)"""
    lib.bvcf_bench_guarded_buffers.restype = C.c_size_t
    lib.bvcf_bench_guarded_buffers.argtypes = []
    return int(lib.bvcf_bench_guarded_buffers())


def string_header(cfg=None):
    c = make_config(cfg)
    buf = C.create_string_buffer(512)
    n = lib.bvcf_string_header(C.byref(c), buf, len(buf))
    return buf.raw[:n].decode()


def run_buffer(vcf_bytes, cfg=None, device=0, max_batch_bytes=0, n_format_threads=0):
    """readVcf on an in-memory VCF through the HIP path.
    -> (rc, TSV body bytes (no header line), log text, n data lines)"""
    # (a Config -- make_config's, or the head of a ConfigMore filled by hand -- is passed on as it is)
    c = cfg if isinstance(cfg, Config) else make_config(cfg, device, max_batch_bytes, n_format_threads)
    out, log = C.c_void_p(), C.c_void_p()
    n_out, n_log, n_lines = C.c_size_t(), C.c_size_t(), C.c_uint64()
    rc = lib.bvcf_run_buffer(C.byref(c), vcf_bytes, len(vcf_bytes), C.byref(out), C.byref(n_out), C.byref(log),
                             C.byref(n_log), C.byref(n_lines))
    o = C.string_at(out, n_out.value) if out.value else b""
    e = C.string_at(log, n_log.value).decode(errors="replace") if log.value else ""
    lib.bvcf_free(out)
    lib.bvcf_free(log)
    return rc, o, e, n_lines.value


def run_fd(fd_in, fd_out, fd_err, cfg=None, device=0, max_batch_bytes=0):
    """bvcf_run_fd over open file descriptors -> (rc, n data lines)"""
    c = make_config(cfg, device, max_batch_bytes)
    n_lines = C.c_uint64()
    rc = lib.bvcf_run_fd(C.byref(c), fd_in, fd_out, fd_err, C.byref(n_lines))
    return rc, n_lines.value


def allreduce_counters(ctxs):
    """the final count gather over a list of Ctx -> (totals[8], used_rccl)"""
    arr = (C.c_void_p * len(ctxs))(*[x.h for x in ctxs])
    out = (C.c_uint64 * 8)()
    used = C.c_int(0)
    rc = lib.bvcf_allreduce_counters(arr, len(ctxs), out, C.byref(used))
    if rc:
        raise BvcfError(rc, lib.bvcf_last_error(ctxs[0].h).decode())
    return list(out), bool(used.value)


lib.bvcf_bgzf_inflate_device.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]


def bgzf_inflate_device(comp, cap=None, device=0):
    """whole BGZF blocks -> (rc, text) through k_inflate / k_crc32 on the device"""
    cap = cap if cap is not None else max(64, 66000 * (comp.count(b"\x1f\x8b\x08\x04") + 1))
    buf = C.create_string_buffer(cap)
    n = C.c_size_t()
    rc = lib.bvcf_bgzf_inflate_device(device, comp, len(comp), buf, cap, C.byref(n))
    return rc, (buf.raw[:n.value] if rc == 0 else b""), n.value


lib.bvcf_bgzf_deflate_device.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]
PIECE = 65280  # text per BGZF member of bgzf_deflate_device / --compressOutput bgzf
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_bound(n):
    """BVCF_BGZF_BOUND(n): the most bgzf_deflate_device can produce for n bytes of text"""
    return (n + PIECE - 1) // PIECE * 65311 + 28


def bgzf_deflate_device(data, add_eof=True, device=0):
    """text -> BGZF members (one per 65 280 bytes) through k_deflate / k_crc32 / k_bgzf_pack on the device"""
    data = bytes(data)
    cap = bgzf_bound(len(data))
    buf = C.create_string_buffer(cap)
    n = C.c_size_t()
    rc = lib.bvcf_bgzf_deflate_device(device, data, len(data), int(bool(add_eof)), buf, cap, C.byref(n))
    if rc:
        raise BvcfError(rc, "bvcf_bgzf_deflate_device")
    return buf.raw[:n.value]


def decompress(data, n_threads=0):
    """gzip / BGZF / plain bytes -> (rc, bytes, kind) through the driver's byte source (host only)"""
    import tempfile
    with tempfile.TemporaryFile() as fi, tempfile.TemporaryFile() as fo:
        fi.write(data)
        fi.flush()
        fi.seek(0)
        kind = C.create_string_buffer(8)
        rc = lib.bvcf_decompress_fd(fi.fileno(), fo.fileno(), n_threads, kind)
        fo.seek(0)
        return rc, fo.read(), kind.value.decode()


def decompress_pipe(data, n_threads=16, piece=0, seed=0):
    """the same through a PIPE (stdin's shape): a writer thread feeds `data` in pieces of `piece` bytes (0: random sizes up
    to 3 MiB) -- text through a pipe is read by bvcf_input's splice fan-out when n_threads allows -> (rc, bytes, kind)"""
    import random
    import tempfile
    import threading
    r, w = os.pipe()
    rng = random.Random(seed)

    def feed():
        try:
            mv, off = memoryview(data), 0
            while off < len(mv):
                n = piece or rng.choice([1, 7, 4096, 65536, 100_000, 1 << 20, 3 << 20])
                off += os.write(w, mv[off:off + n])
        finally:
            os.close(w)

    t = threading.Thread(target=feed)
    t.start()
    try:
        with tempfile.TemporaryFile() as fo:
            kind = C.create_string_buffer(8)
            rc = lib.bvcf_decompress_fd(r, fo.fileno(), n_threads, kind)
            fo.seek(0)
            return rc, fo.read(), kind.value.decode()
    finally:
        os.close(r)
        t.join()


class Batch:
    """numpy views (copied) of one collected bvcf_result"""

    def __init__(self, r):
        self.batch_seq = r.batch_seq
        # bvcf_site_gate_count, SITE_GATE_REPORT's seven counts of this batch: counted when asked for (gate_counts), from
        # the record arrays as they are now -- like every view here they belong to the slot, valid until it takes another batch
        self._result = r
        self._gate_counts = None
        self._variant_counts = None  # bvcf_variant_gate_count, likewise
        self._region_counts = None  # bvcf_region_gate_count, likewise
        self.n_samples = r.n_samples
        self.cmap_stride = r.cmap_stride
        self.kernel_ms = r.kernel_ms
        self.n_lines_seen = r.n_lines_seen

        def arr(ptr, n, dt):
            if not n:
                return np.zeros(0, dtype=dt)
            return np.frombuffer(C.string_at(ptr, n * dt.itemsize), dtype=dt).copy()

        self.sites = None
        # bvcf_params.render_sites: the rows of the lines the packed form settles, and where the other lines' rows belong
        self.rows = C.string_at(r.rows, r.n_row_bytes) if r.rows and r.n_row_bytes else b""
        self.row_cuts = arr(r.row_cuts, r.n_row_cuts, ROW_CUT_DTYPE) if r.row_cuts else np.zeros(0, dtype=ROW_CUT_DTYPE)
        self.n_ok_sites = r.n_ok_sites
        self.rendered = bool(r.rows) or (not r.sites and r.n_row_cuts > 0) or bool(r.n_ok_sites)
        if r.sites:
            # the packed form of a file without samples (bvcf_params.packed_sites): expanded here into the arrays of the full
            # form, so that line i is lines[i] and its first record alleles[i] whichever way the batch came back
            self.sites = arr(r.sites, r.n_lines, SITE_DTYPE)
            self.full_lines = arr(r.lines, r.n_full_lines, LINE_DTYPE)
            raw = arr(r.alleles, r.n_alleles, ALLELE_DTYPE)
            self.lines, self.alleles = self._expand(self.sites, self.full_lines, raw, r.n_lines)
        elif r.row_cuts:
            # rendered rows (bvcf_params.render_sites): only the lines left to the host have records -- lines[cut.slot]
            self.full_lines = arr(r.lines, r.n_full_lines, LINE_DTYPE)
            self.lines = self.full_lines
            self.alleles = arr(r.alleles, r.n_alleles, ALLELE_DTYPE)
        else:
            self.lines = arr(r.lines, r.n_lines, LINE_DTYPE)
            self.alleles = arr(r.alleles, r.n_alleles, ALLELE_DTYPE)
        self.n_lines = r.n_lines
        self.errs = arr(r.errs, r.n_errs, ERR_DTYPE)
        self.cmap = arr(r.cmap, r.n_cmap_bytes, np.dtype("u1"))
        # want_dosage: one int8 row per alleles[] slot (rows of slots without a record hold garbage)
        # bvcf_submit_bgzf: the batch's inflated text (lines[].off point into it)
        self.text = C.string_at(r.text, r.n_text_bytes) if r.text and r.n_text_bytes else b""
        # ... with samples only the line heads (CHROM..INFO), packed: line i's bytes start at text[head_off[i]]
        self.head_off = arr(r.head_off, r.n_lines, np.dtype("<u4")) if r.head_off else None
        # want_name_lists: (off[3], len[3]) per alleles[] slot into the text arena `names`
        self.name_lists = arr(r.name_lists, r.n_alleles, NAMES_DTYPE) if r.name_lists else None
        self.names = C.string_at(r.names, r.n_name_bytes) if r.names and r.n_name_bytes else b""
        self.dosage = None
        if r.dosage and r.n_alleles:
            self.dosage = arr(r.dosage, r.n_alleles * r.dosage_stride, np.dtype("i1")).reshape(r.n_alleles, r.dosage_stride)

    @staticmethod
    def _expand(sites, full_lines, raw_alleles, n):
        lines = np.zeros(n, dtype=LINE_DTYPE)
        # the batch's alleles[]: the n_full first records, the further alleles right behind them (rec_first points there);
        # expanded: slot i for line i, the further alleles behind the n lines
        n_full = len(full_lines)
        extras = raw_alleles[n_full:]
        alleles = np.concatenate([np.zeros(n, dtype=ALLELE_DTYPE), extras])
        full = (sites["status"] & SITE_FULL) != 0
        fi = sites["full_idx"][full]
        assert len(set(fi.tolist())) == len(fi) and (fi < n_full).all(), "full_idx: distinct slots below n_full_lines"
        moved = full_lines.copy()
        multi = moved["n_rec"] > 1
        assert (moved["rec_first"][multi] >= n_full).all() and (moved["rec_first"][multi] + moved["n_rec"][multi] - 1 <= len(raw_alleles)).all()
        moved["rec_first"][multi] = moved["rec_first"][multi] - n_full + n
        lines[full] = moved[fi]
        assert (full_lines[fi]["gt_task"] == np.nonzero(full)[0]).all(), "a full record names its line"
        firsts = raw_alleles[fi].copy()
        # packed lines: a SNP with its position taken verbatim (or a line that failed the gate: no record)
        pk = ~full
        lines["off"][pk] = sites["off"][pk]
        lines["len"][pk] = sites["len"][pk]
        fe = sites["fend"].astype(np.uint32)
        fe9 = np.concatenate([fe, np.full((n, 1), 0xFF, dtype=np.uint32)], axis=1)
        fe9 = np.where(fe9 == 0xFF, sites["len"][:, None], fe9)
        lines["fend"][pk] = fe9[pk]
        lines["n_rec"][pk] = (sites["status"][pk] == LINE_OK).astype(np.uint32)
        lines["n_fields"][pk] = sites["n_fields"][pk]
        lines["gt_task"][pk] = np.nonzero(pk)[0]
        lines["status"][pk] = sites["status"][pk]
        idx = np.nonzero(pk)[0]
        alleles["line"][idx] = idx
        alleles["alt_len"][idx] = 1
        alleles["cmap_off"][idx] = NO_CMAP
        alleles["ref"][idx] = sites["ref"][pk]
        alleles["alt_base"][idx] = sites["alt_base"][pk]
        alleles["trtv"][idx] = sites["trtv"][pk]
        alleles["flags"][idx] = 1
        alleles["gt_task"][idx] = 0xFFFFFFFF
        alleles[np.nonzero(full)[0]] = firsts
        return lines, alleles

    def records(self, i):
        """the output alleles of line i, in order"""
        L = self.lines[i]
        n = int(L["n_rec"])
        if n == 0:
            return self.alleles[:0]
        idx = [i] + [int(L["rec_first"]) + j - 1 for j in range(1, n)]
        return self.alleles[idx]

    @property
    def gate_counts(self):
        if self._gate_counts is None:
            self._gate_counts = site_gate_count(self._result)
        return self._gate_counts

    @property
    def variant_counts(self):
        if self._variant_counts is None:
            self._variant_counts = variant_gate_count(self._result)
        return self._variant_counts

    @property
    def region_counts(self):
        if self._region_counts is None:
            self._region_counts = region_gate_count(self._result)
        return self._region_counts

    def record_slots(self, i):
        """indices into alleles[] (and dosage[]) of line i's output alleles, in order"""
        L = self.lines[i]
        n = int(L["n_rec"])
        return [] if n == 0 else [i] + [int(L["rec_first"]) + j - 1 for j in range(1, n)]

    def line_head(self, i):
        """the bytes of line i that came back with a bvcf_submit_bgzf batch: the whole line (no samples) or its head up
        to the end of the INFO column"""
        L = self.lines[i]
        if self.head_off is None:
            return self.text[int(L["off"]):int(L["off"]) + int(L["len"])]
        n = min(int(L["fend"][7]), int(L["len"]))
        return self.text[int(self.head_off[i]):int(self.head_off[i]) + n]

    def name_list(self, slot, q):
        """list q (0 het, 1 hom, 2 missing) of alleles[slot] as the device rendered it"""
        nl = self.name_lists[slot]
        return self.names[int(nl["off"][q]):int(nl["off"][q]) + int(nl["len"][q])]

    def classes(self, allele_row):
        """per-sample class codes (0 none, 1 het, 2 hom, 3 missing) of one allele record"""
        off = int(allele_row["cmap_off"])
        ns = self.n_samples
        if int(allele_row["flags"]) & 2:  # BVCF_ALLELE_CMAP_SPARSE: count, then (byte index << 8 | byte) entries
            words = self.cmap[off:off + 64].view("<u4")
            m = np.zeros((ns + 3) // 4, dtype=np.uint8)
            for e in words[1:1 + int(words[0])]:
                m[int(e) >> 8] = int(e) & 0xFF
        else:
            m = self.cmap[off:off + (ns + 3) // 4]
        return ((m[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(-1)[:ns]


class Ctx:
    """one bvcf_ctx (one GPU)"""

    def __init__(self, n_header_fields, allow="PASS,.", exclude="", device=0, eol_chars=1, eol_byte=b"\n",
                 max_batch_bytes=0, max_lines=0, max_alleles=0, cmap_bytes=0, n_slots=0, want_class_maps=True,
                 path=0, want_dosage=False, sample_names=None, delimiter=";", packed_sites=False, render_sites=False,
                 empty_field="!", keep_pos=False, keep_id=False, keep_info=False, sample_stats=False,
                 min_gq=0, min_dp=0, sample_keep=None, pair_stats=False, site_gate=None, bed_rows=False, trios=None, ld=None,
                 variants=None, regions=None, grm=False, score=None, pheno=None, covar=None, logit=None):
        p = make_params(n_header_fields, allow, exclude, device, eol_chars, eol_byte, max_batch_bytes, max_lines, max_alleles,
                        cmap_bytes, n_slots, want_class_maps, path, want_dosage, sample_names is not None, packed_sites,
                        render_sites, sample_stats, min_gq, min_dp, sample_keep)
        self.n_samples = max(n_header_fields - 9, 0)
        if sample_keep is not None:  # (n_samples = the number of kept samples)
            self.n_samples = len(set(int(s) for s in sample_keep if 0 <= int(s) < self.n_samples))
        self.h = C.c_void_p()
        rc = lib.bvcf_create(C.byref(self.h), C.byref(p))
        if rc:
            raise BvcfError(rc, lib.bvcf_last_error(None).decode())
        if pair_stats:  # bvcf_enable_pair_stats: the pair tables behind every chain (read with pair_stats())
            lib.bvcf_enable_pair_stats.argtypes = [C.c_void_p]
            rc = lib.bvcf_enable_pair_stats(self.h)
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
        self.score_columns = 0
        if score is not None:  # bvcf_set_score_table: a built ScoreTable; the scores' words behind every chain (score_words())
            lib.bvcf_set_score_table.argtypes = [C.c_void_p, C.c_void_p]
            rc = lib.bvcf_set_score_table(self.h, C.byref(score.t))
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
            self.score_columns = score.n_columns
        self.assoc_columns = 0
        if pheno is not None:  # bvcf_set_pheno_table: a built PhenoTable; the scan's records behind every chain (assoc())
            lib.bvcf_set_pheno_table.argtypes = [C.c_void_p, C.c_void_p]
            rc = lib.bvcf_set_pheno_table(self.h, C.byref(pheno.t))
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
            self.assoc_columns = pheno.n_columns
        if covar is not None:  # bvcf_set_covar_table: a CovarTable bound to pheno; the covariate records beside (assoc_cov())
            lib.bvcf_set_covar_table.argtypes = [C.c_void_p, C.c_void_p]
            rc = lib.bvcf_set_covar_table(self.h, C.byref(covar.t))
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
        if logit is not None:  # bvcf_set_logit_table: a LogitTable built from pheno; the logistic records beside (assoc_logit())
            lib.bvcf_set_logit_table.argtypes = [C.c_void_p, C.c_void_p]
            rc = lib.bvcf_set_logit_table(self.h, C.byref(logit.t))
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
        if grm:  # bvcf_enable_grm: the GRM's integer tables behind every chain (read with grm() / grm_words())
            lib.bvcf_enable_grm.argtypes = [C.c_void_p]
            rc = lib.bvcf_enable_grm(self.h)
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
        if bed_rows:  # bvcf_enable_bed_rows: the .bed rows behind every chain (read with bed_rows() after each collect)
            lib.bvcf_enable_bed_rows.argtypes = [C.c_void_p]
            rc = lib.bvcf_enable_bed_rows(self.h)
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
        if trios is not None:  # bvcf_enable_trios: (child, father, mother) kept-sample indices (read with trio_stats() after each collect)
            t = np.ascontiguousarray(np.asarray(trios, dtype=np.uint32).reshape(-1, 3))
            lib.bvcf_enable_trios.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            rc = lib.bvcf_enable_trios(self.h, t.ctypes.data if len(t) else None, len(t))
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
        if ld is not None:  # bvcf_enable_ld: (window, t6) (read with ld_stats() after each collect)
            lib.bvcf_enable_ld.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
            rc = lib.bvcf_enable_ld(self.h, int(ld[0]), int(ld[1]))
            if rc:
                msg = lib.bvcf_last_error(self.h).decode()
                self.close()
                raise BvcfError(rc, msg)
        if regions is not None:  # bvcf_set_region_table: a built RegionTable
            try:
                self.set_region_table(regions)
            except BvcfError:
                self.close()
                raise
        if variants is not None:  # bvcf_set_variant_list / bvcf_set_variant_table: (loci or a VariantTable, exclude)
            try:
                self.set_variant_list(*variants)
            except BvcfError:
                self.close()
                raise
        if site_gate is not None:  # bvcf_set_site_gate: a SiteGate, or make_site_gate's keywords as a dict
            try:
                self.set_site_gate(site_gate)
            except BvcfError:
                self.close()
                raise
        if render_sites:
            lib.bvcf_set_row_format.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
            self._check(lib.bvcf_set_row_format(self.h, empty_field.encode(), int(keep_pos), int(keep_id), int(keep_info)))
        if sample_names is not None:  # device-side rendering of the het / hom / missing name lists
            enc = [x.encode() if isinstance(x, str) else x for x in sample_names]
            ptrs = (C.c_char_p * max(len(enc), 1))(*enc)
            lens = (C.c_uint32 * max(len(enc), 1))(*[len(x) for x in enc])
            self._check(lib.bvcf_set_sample_names(self.h, ptrs, lens, len(enc), delimiter.encode()))

    def close(self):
        if self.h:
            lib.bvcf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise BvcfError(rc, lib.bvcf_last_error(self.h).decode())

    def submit(self, block, seq=0):
        self._blk = block  # keep alive until collect
        self._check(lib.bvcf_submit(self.h, block, len(block), seq))

    def submit_bgzf(self, comp, n_own, skip_first_line, first_off=0, seq=0):
        """whole BGZF blocks: n_own bytes of own blocks, then look-ahead blocks (see include/bvcf.h)"""
        self._blk = comp
        self._check(lib.bvcf_submit_bgzf(self.h, comp, len(comp), n_own, int(skip_first_line), first_off, seq))

    def submit_device(self, dptr, nbytes, seq=0):
        self._check(lib.bvcf_submit_device(self.h, dptr, nbytes, seq))

    def reserve(self, lines, alleles, cmap_bytes):
        self._check(lib.bvcf_reserve(self.h, lines, alleles, cmap_bytes))

    def collect(self, tsv=None):
        """the oldest batch in flight.  tsv = (block, cfg, sample_names): also its TSV rows and log lines through
        bvcf_format_tsv, made from the raw result before its slot can take another batch -> Batch.tsv (bytes) and
        Batch.log (text).  block: the host bytes of the submitted block (any buffer; a memoryview slice is not copied),
        cfg: a make_config dict or Config, sample_names: the normalised header fields 9.."""
        r = Result()
        rc = lib.bvcf_collect(self.h, C.byref(r))
        if rc == E_CAPACITY:
            raise BvcfError(rc, "capacity: need lines=%d alleles=%d cmap=%d" % (r.need_lines, r.need_alleles, r.need_cmap_bytes))
        self._check(rc)
        if tsv is None:
            return Batch(r)
        block, cfg, names = tsv
        c = cfg if isinstance(cfg, Config) else make_config(cfg)
        buf = np.frombuffer(block, dtype=np.uint8)
        enc = [x.encode() if isinstance(x, str) else x for x in (names or [])]
        ptrs = (C.c_char_p * max(len(enc), 1))(*enc)
        lens = (C.c_uint32 * max(len(enc), 1))(*[len(x) for x in enc])
        out, log = C.c_void_p(), C.c_void_p()
        n_out, n_log = C.c_size_t(), C.c_size_t()
        rc = lib.bvcf_format_tsv(C.byref(c), C.byref(r), buf.ctypes.data if len(buf) else None, ptrs, lens, C.byref(out),
                                 C.byref(n_out), C.byref(log), C.byref(n_log))
        try:
            if rc:
                raise BvcfError(rc, "bvcf_format_tsv")
            text = C.string_at(out, n_out.value) if out.value else b""
            log_text = C.string_at(log, n_log.value).decode(errors="replace") if log.value else ""
        finally:
            lib.bvcf_free(out)
            lib.bvcf_free(log)
        b = Batch(r)
        b.tsv, b.log = text, log_text
        return b

    def process(self, block):
        self.submit(block)
        return self.collect()

    def bench_device(self, dptrs, nbytes, iters, slots=0):
        """kernel chain `iters` times over resident blocks (rotating); results stay on the device.  Batch i runs on
        slot i % slots (0 = all of the ctx's slots; 1 = strictly one batch after the other).
        -> (chain ms per batch, genotype-scan ms per batch, [lines, alleles, errs, cmap bytes, tasks])"""
        n = len(dptrs)
        ptrs = (C.c_void_p * n)(*dptrs)
        sizes = (C.c_size_t * n)(*nbytes)
        chain = (C.c_float * iters)()
        scan = (C.c_float * iters)()
        counts = (C.c_uint64 * 5)()
        self._check(lib.bvcf_bench_device_slots(self.h, ptrs, sizes, n, iters, slots, chain, scan, counts))
        return list(chain), list(scan), list(counts)

    def path(self):
        """1 = census path, 2 = streaming path"""
        return lib.bvcf_path(self.h)

    def stream_kernel(self):
        """the streaming kernel the next batch goes through: "k_stream", "k_stream_gen", or None off the streaming path"""
        lib.bvcf_bench_stream_kernel.argtypes = [C.c_void_p]
        lib.bvcf_bench_stream_kernel.restype = C.c_int
        k = lib.bvcf_bench_stream_kernel(self.h)
        return None if k < 0 else ("k_stream_gen" if k else "k_stream")

    def head_left(self):
        """streaming path: the lines of the last collected batch that k_order left to k_head (None: no batch yet, or not
        on the streaming path)"""
        lib.bvcf_bench_head_left.argtypes = [C.c_void_p]
        lib.bvcf_bench_head_left.restype = C.c_long
        n = lib.bvcf_bench_head_left(self.h)
        return None if n < 0 else int(n)

    def sample_stats(self, reset=False):
        """bvcf_params.want_sample_stats: the per-sample counts over the rows of the batches collected so far ->
        uint64 array (n_samples, 6): het, hom, missing, transitions, transversions, rows (see include/bvcf.h)"""
        out = np.zeros(6 * self.n_samples, dtype=np.uint64)
        lib.bvcf_sample_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self._check(lib.bvcf_sample_stats(self.h, out.ctypes.data if self.n_samples else None, int(reset)))
        return out.reshape(6, self.n_samples).T.copy()

    def set_site_gate(self, gate):
        """bvcf_set_site_gate, before the first submit: gate is a SiteGate or make_site_gate's keywords as a dict"""
        g = gate if isinstance(gate, SiteGate) else make_site_gate(**gate)
        lib.bvcf_set_site_gate.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_set_site_gate(self.h, C.byref(g)))

    def set_variant_list(self, loci, exclude=False):
        """before the first submit: loci is a list of locus strings (bytes; bvcf_set_variant_list) or a built VariantTable
        (bvcf_set_variant_table); exclude: the listed rows go instead of staying"""
        if isinstance(loci, VariantTable):
            lib.bvcf_set_variant_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            self._check(lib.bvcf_set_variant_table(self.h, C.byref(loci.t), int(bool(exclude))))
            return
        loci = [bytes(x) for x in loci]
        blob = b"".join(loci)
        lens = np.array([len(x) for x in loci], dtype=np.uint32)
        offs = np.zeros(len(loci), dtype=np.uint64)
        if len(loci) > 1:
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        lib.bvcf_set_variant_list.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        self._check(lib.bvcf_set_variant_list(self.h, blob, offs.ctypes.data if len(loci) else None,
                                              lens.ctypes.data if len(loci) else None, len(loci), int(bool(exclude))))

    def set_region_table(self, table):
        """before the first submit: a built RegionTable (bvcf_set_region_table)"""
        lib.bvcf_set_region_table.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_set_region_table(self.h, C.byref(table.t)))

    def region_gate_stride(self):
        """the alleles[] slots k_region_gate's grid covers in one step"""
        lib.bvcf_bench_region_gate_stride.restype = C.c_uint32
        lib.bvcf_bench_region_gate_stride.argtypes = [C.c_void_p]
        return int(lib.bvcf_bench_region_gate_stride(self.h))

    def bench_region_kernel(self):
        """k_region_gate over the last bench block of the ctx -> ms"""
        ms = C.c_float()
        lib.bvcf_bench_region_kernel.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_bench_region_kernel(self.h, C.byref(ms)))
        return float(ms.value)

    def variant_gate_stride(self):
        """the alleles[] slots k_variant_gate's grid covers in one step"""
        lib.bvcf_bench_variant_gate_stride.restype = C.c_uint32
        lib.bvcf_bench_variant_gate_stride.argtypes = [C.c_void_p]
        return int(lib.bvcf_bench_variant_gate_stride(self.h))

    def bench_variant_kernel(self):
        """k_variant_gate over the last bench block of the ctx -> ms"""
        ms = C.c_float()
        lib.bvcf_bench_variant_kernel.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_bench_variant_kernel(self.h, C.byref(ms)))
        return float(ms.value)

    def bed_rows_info(self):
        """bvcf_bed_rows: the BedRowsInfo of the batch collected last (need_bytes is set after BVCF_E_CAPACITY too)"""
        info = BedRowsInfo()
        lib.bvcf_bed_rows.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_bed_rows(self.h, C.byref(info)))
        return info

    def bed_rows(self):
        """the .bed rows of the batch collected last -> a uint8 array (n_rows, row_bytes), copied out of the slot"""
        info = self.bed_rows_info()
        n = int(info.n_rows) * int(info.row_bytes)
        if not n:
            return np.zeros((0, int(info.row_bytes)), dtype=np.uint8)
        buf = (C.c_uint8 * n).from_address(info.rows)
        return np.frombuffer(buf, dtype=np.uint8).reshape(int(info.n_rows), int(info.row_bytes)).copy()

    def reserve_bed_rows(self, nbytes):
        """bvcf_reserve_bed_rows: grow the arena of the .bed rows (no batch in flight)"""
        lib.bvcf_reserve_bed_rows.argtypes = [C.c_void_p, C.c_uint64]
        self._check(lib.bvcf_reserve_bed_rows(self.h, int(nbytes)))

    def trio_info(self):
        """bvcf_trio_stats: the TrioInfo of the batch collected last (need_events is set after BVCF_E_CAPACITY too)"""
        info = TrioInfo()
        lib.bvcf_trio_stats.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_trio_stats(self.h, C.byref(info)))
        return info

    def trio_stats(self):
        """the batch collected last -> (counts uint32 (n_trios, 3): informative, errors, denovo; events uint32 (n_events, 5):
        row, trio, then the classes of child, father and mother), copied out of the slot"""
        info = self.trio_info()
        nt, ne = int(info.n_trios), int(info.n_events)
        counts = np.zeros((nt, 3), dtype=np.uint32)
        if nt and info.counts:
            counts = np.frombuffer((C.c_uint32 * (3 * nt)).from_address(info.counts), dtype=np.uint32).reshape(nt, 3).copy()
        ev = np.zeros((ne, 5), dtype=np.uint32)
        if ne:
            raw = np.frombuffer((C.c_uint32 * (2 * ne)).from_address(info.events), dtype=np.uint32).reshape(ne, 2)
            w = raw[:, 1]
            ev = np.stack([raw[:, 0], w & 0xFFFFFF, (w >> 24) & 3, (w >> 26) & 3, (w >> 28) & 3], axis=1).astype(np.uint32)
        return counts, ev

    def reserve_trio_events(self, n):
        """bvcf_reserve_trio_events: grow the arena of the events (no batch in flight)"""
        lib.bvcf_reserve_trio_events.argtypes = [C.c_void_p, C.c_uint64]
        self._check(lib.bvcf_reserve_trio_events(self.h, int(n)))

    def ld_info(self):
        """bvcf_ld_stats: the LdInfo of the batch collected last (need_events is set after BVCF_E_CAPACITY too)"""
        info = LdInfo()
        lib.bvcf_ld_stats.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_ld_stats(self.h, C.byref(info)))
        return info

    def ld_stats(self):
        """the batch collected last -> (events uint32 (n_events, 8): b, d, n, sa, sb, saa, sbb, sab; head rows and tail rows
        uint8 (n_edge, row_bytes) in .bed code; rows of the batch), copied out of the slot"""
        info = self.ld_info()
        ne, k, rb = int(info.n_events), int(info.n_edge), int(info.row_bytes)
        ev = np.zeros((ne, 8), dtype=np.uint32)
        if ne:
            ev = np.frombuffer((C.c_uint32 * (8 * ne)).from_address(info.events), dtype=np.uint32).reshape(ne, 8).copy()
        head = tail = np.zeros((0, rb), dtype=np.uint8)
        if k and rb:
            head = np.frombuffer((C.c_uint8 * (k * rb)).from_address(info.head_rows), dtype=np.uint8).reshape(k, rb).copy()
            tail = np.frombuffer((C.c_uint8 * (k * rb)).from_address(info.tail_rows), dtype=np.uint8).reshape(k, rb).copy()
        return ev, head, tail, int(info.n_rows)

    def reserve_ld_events(self, n):
        """bvcf_reserve_ld_events: grow the arena of the events (no batch in flight)"""
        lib.bvcf_reserve_ld_events.argtypes = [C.c_void_p, C.c_uint64]
        self._check(lib.bvcf_reserve_ld_events(self.h, int(n)))

    def bench_ld_kernels(self):
        """the LD kernels over the first slot's last bench chain -> (ms of [row index, k_bed_rows, k_ld_keys, k_ld_pairs
        counting, k_ld_scan, k_ld_pairs filling], rows, events)"""
        ms = (C.c_float * 6)()
        out = (C.c_uint64 * 2)()
        lib.bvcf_bench_ld_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(lib.bvcf_bench_ld_kernels(self.h, ms, out))
        return list(ms), int(out[0]), int(out[1])

    def bench_trio_kernels(self):
        """the trio kernels over the first slot's last bench chain -> (ms of [row index + memsets, k_trio_count, k_trio_scan,
        k_trio_fill], rows, events)"""
        ms = (C.c_float * 4)()
        out = (C.c_uint64 * 2)()
        lib.bvcf_bench_trio_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(lib.bvcf_bench_trio_kernels(self.h, ms, out))
        return list(ms), int(out[0]), int(out[1])

    def bench_bed_kernels(self):
        """the .bed kernels over the first slot's last bench chain -> (ms of [k_bed_count + k_bed_scan + k_bed_index, k_bed_rows], rows, bytes)"""
        ms = (C.c_float * 2)()
        out = (C.c_uint64 * 2)()
        lib.bvcf_bench_bed_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(lib.bvcf_bench_bed_kernels(self.h, ms, out))
        return list(ms), int(out[0]), int(out[1])

    def bench_gate_kernels(self):
        """the gate kernels over the last bench block of the ctx -> ms of [k_site_gate, k_site_hwe]"""
        ms = (C.c_float * 2)()
        lib.bvcf_bench_gate_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(lib.bvcf_bench_gate_kernels(self.h, ms))
        return list(ms)

    def bench_pair_kernels(self):
        """the pair kernels over the first slot's last bench chain -> ms of [k_pr_planes, k_pr_gemm, k_pr_sparse, k_pr_fold]"""
        ms = (C.c_float * 4)()
        lib.bvcf_bench_pair_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(lib.bvcf_bench_pair_kernels(self.h, ms))
        return list(ms)

    def bench_grm_kernels(self):
        """the GRM kernels over the first slot's last bench chain -> ms of [k_grm_list, k_grm_pack + k_grm_gemm, k_grm_sparse, k_grm_fold]"""
        ms = (C.c_float * 4)()
        lib.bvcf_bench_grm_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(lib.bvcf_bench_grm_kernels(self.h, ms))
        return list(ms)

    def bench_assoc_kernels(self):
        """the scan's kernels over the first slot's last bench chain -> ms of [k_assoc_list, k_assoc_gemm, k_assoc_sparse]"""
        ms = (C.c_float * 3)()
        lib.bvcf_bench_assoc_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(lib.bvcf_bench_assoc_kernels(self.h, ms))
        return list(ms)

    def assoc_info(self):
        """bvcf_assoc: the AssocInfo of the batch collected last (need_rows is set after BVCF_E_CAPACITY too)"""
        info = AssocInfo()
        lib.bvcf_assoc.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_assoc(self.h, C.byref(info)))
        return info

    def assoc(self):
        """the batch collected last -> its records, an ASSOC_REC_DTYPE array (n_rows, K), copied out of the slot"""
        info = self.assoc_info()
        n, k = int(info.n_rows), int(info.n_columns)
        if not n or not info.recs:
            return np.zeros((0, k), dtype=ASSOC_REC_DTYPE)
        raw = (C.c_uint8 * (n * k * ASSOC_REC_DTYPE.itemsize)).from_address(info.recs)
        return np.frombuffer(raw, dtype=ASSOC_REC_DTYPE).reshape(n, k).copy()

    def assoc_cov(self):
        """bvcf_assoc_cov: the batch collected last -> its covariate records, uint64 (n_rows, row_words), copied out of the slot"""
        info = AssocCovInfo()
        lib.bvcf_assoc_cov.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_assoc_cov(self.h, C.byref(info)))
        n, w = int(info.n_rows), int(info.row_words)
        if not n or not info.words:
            return np.zeros((0, w), dtype=np.uint64)
        raw = (C.c_uint8 * (n * w * 8)).from_address(info.words)
        return np.frombuffer(raw, dtype=np.uint64).reshape(n, w).copy()

    def assoc_logit(self):
        """bvcf_assoc_logit: the batch collected last -> its logistic records, uint64 (n_rows, row_words), copied out of the slot"""
        info = AssocLogitInfo()
        lib.bvcf_assoc_logit.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib.bvcf_assoc_logit(self.h, C.byref(info)))
        n, w = int(info.n_rows), int(info.row_words)
        if not n or not info.words:
            return np.zeros((0, w), dtype=np.uint64)
        raw = (C.c_uint8 * (n * w * 8)).from_address(info.words)
        return np.frombuffer(raw, dtype=np.uint64).reshape(n, w).copy()

    def bench_assoc_logit_kernels(self):
        """the logistic kernels over the first slot's last bench chain -> ms of [k_assoc_logit_gemm, k_assoc_logit_sparse]"""
        ms = (C.c_float * 2)()
        lib.bvcf_bench_assoc_logit_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(lib.bvcf_bench_assoc_logit_kernels(self.h, ms))
        return list(ms)

    def bench_assoc_cov_kernels(self):
        """the covariate kernels over the first slot's last bench chain -> ms of [k_assoc_cov_gemm, k_assoc_cov_sparse]"""
        ms = (C.c_float * 2)()
        lib.bvcf_bench_assoc_cov_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(lib.bvcf_bench_assoc_cov_kernels(self.h, ms))
        return list(ms)

    def reserve_assoc_rows(self, n):
        """bvcf_reserve_assoc_rows: grow the arena of the records (no batch in flight)"""
        lib.bvcf_reserve_assoc_rows.argtypes = [C.c_void_p, C.c_uint64]
        self._check(lib.bvcf_reserve_assoc_rows(self.h, int(n)))

    def bench_score_kernels(self):
        """the score kernels over the first slot's last bench chain -> ms of [k_score_list, k_score_gemm, k_score_sparse, k_score_fold]"""
        ms = (C.c_float * 4)()
        lib.bvcf_bench_score_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(lib.bvcf_bench_score_kernels(self.h, ms))
        return list(ms)

    def score_words(self, reset=False):
        """bvcf_set_score_table: the scores over the rows of the batches collected so far, as bvcf_score gives them ->
        (lo, hi, G, X, R): the low and the high 64 bits of T (two's complement) as uint64 arrays (n_samples, K), G and X as
        uint64 arrays (n_samples), R the number of matched rows (see include/bvcf.h)"""
        ns, k = self.n_samples, self.score_columns
        n = ns * k
        out = np.zeros(2 * n + 2 * ns + 1, dtype=np.uint64)
        lib.bvcf_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self._check(lib.bvcf_score(self.h, out.ctypes.data, int(reset)))
        return (out[:n].reshape(ns, k), out[n:2 * n].reshape(ns, k), out[2 * n:2 * n + ns].copy(),
                out[2 * n + ns:2 * n + 2 * ns].copy(), int(out[2 * n + 2 * ns]))

    def scores(self, reset=False):
        """the same with T as a list of rows of Python integers -> (T, G, X, R)"""
        lo, hi, g, x, r = self.score_words(reset)
        t = []
        for lrow, hrow in zip(lo.tolist(), hi.tolist()):
            row = []
            for l, h in zip(lrow, hrow):
                v = (h << 64) | l
                row.append(v - (1 << 128) if v >> 127 else v)
            t.append(row)
        return t, g.tolist(), x.tolist(), r

    def grm_words(self, reset=False):
        """bvcf_enable_grm: the GRM's tables over the rows of the batches collected so far, as bvcf_grm gives them ->
        (lo, hi, MM, N): the low and the high 64 bits of T (two's complement) and MM as uint64 arrays (n_samples,
        n_samples), N the number of GRM rows (see include/bvcf.h)"""
        ns = self.n_samples
        n = ns * ns
        out = np.zeros(3 * n + 1, dtype=np.uint64)
        lib.bvcf_grm.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self._check(lib.bvcf_grm(self.h, out.ctypes.data, int(reset)))
        return out[:n].reshape(ns, ns), out[n:2 * n].reshape(ns, ns), out[2 * n:3 * n].reshape(ns, ns), int(out[3 * n])

    def grm(self, reset=False):
        """the same with T as an object array of Python integers -> (T, MM, N)"""
        lo, hi, mm, n = self.grm_words(reset)
        t = np.empty(lo.size, dtype=object)
        for k, (l, h) in enumerate(zip(lo.ravel().tolist(), hi.ravel().tolist())):
            v = (h << 64) | l
            t[k] = v - (1 << 128) if v >> 127 else v
        return t.reshape(lo.shape), mm, n

    def pair_stats(self, reset=False):
        """bvcf_enable_pair_stats: the pair tables over the rows of the batches collected so far -> uint64 array
        (3, n_samples, n_samples): HH, OC, HM (see include/bvcf.h)"""
        ns = self.n_samples
        out = np.zeros(3 * ns * ns, dtype=np.uint64)
        lib.bvcf_pair_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self._check(lib.bvcf_pair_stats(self.h, out.ctypes.data if ns else None, int(reset)))
        return out.reshape(3, ns, ns)

    def counters(self):
        out = (C.c_uint64 * 8)()
        self._check(lib.bvcf_counters(self.h, out))
        return list(out)
