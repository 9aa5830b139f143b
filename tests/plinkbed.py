"""--plinkOutput: the expected PREFIX.bed / .bim / .fam, built from the oracle's TSV of the same bytes (numpy only).

The oracle does not know the flag.  A row of its TSV names samples in heterozygotes / homozygotes / missingGenos
(pairtable.matrices: three 0/1 matrices H, O, M, rows x samples); the .bed code of a sample follows the list that names it

    homozygotes 00     missingGenos 01     heterozygotes 10     none of the lists 11

(A1 = the row's ALT, A2 = its REF; a haploid call counts as hom, as in the TSV), sample s in byte s // 4 at bits
2 * (s % 4), ceil(S / 4) bytes per row, the unused high bits of the last byte 0, after the magic 6C 1B 01.  The recode
here is written from that table, not from the library.  Test infrastructure only."""
import random

import numpy as np

import pairtable as pt
import vcfgen

MAGIC = b"\x6c\x1b\x01"
CODE_HOM, CODE_MISSING, CODE_HET, CODE_NONE = 0, 1, 2, 3
# the library's class numbers (BVCF_CLS_*) -> code: the same table, for maps handed to the exported per-row function
CLASS_TO_CODE = {0: CODE_NONE, 1: CODE_HET, 2: CODE_HOM, 3: CODE_MISSING}


def row_bytes(ns):
    return (ns + 3) // 4


def pack_codes(codes):
    """(rows, S) array of 2-bit codes -> (rows, ceil(S / 4)) uint8, the pad bits zero"""
    codes = np.asarray(codes, dtype=np.uint8)
    n, ns = codes.shape
    rb = row_bytes(ns)
    padded = np.zeros((n, 4 * rb), dtype=np.uint8)
    padded[:, :ns] = codes
    q = padded.reshape(n, rb, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def codes_of(H, O, M):
    """the (rows, S) codes of the three list matrices"""
    assert int((H.astype(np.uint16) + O + M).max(initial=0)) <= 1, "a sample is named in two lists of one row"
    codes = np.full(H.shape, CODE_NONE, dtype=np.uint8)
    codes[H == 1] = CODE_HET
    codes[O == 1] = CODE_HOM
    codes[M == 1] = CODE_MISSING
    return codes


def bed_bytes(H, O, M):
    return MAGIC + pack_codes(codes_of(H, O, M)).tobytes()


def decode_bed(bed, ns):
    """a .bed file's bytes -> (H, O, M) uint8 matrices, rows x samples (the inverse of bed_bytes; checks magic, length and
    the pad bits)"""
    assert bed[:3] == MAGIC, bed[:3]
    rb = row_bytes(ns)
    body = np.frombuffer(bed[3:], dtype=np.uint8)
    if ns == 0:
        assert len(body) == 0
        return tuple(np.zeros((0, 0), dtype=np.uint8) for _ in range(3))
    assert len(body) % rb == 0, (len(body), rb)
    rows = body.reshape(-1, rb)
    codes = np.stack([(rows >> (2 * q)) & 3 for q in range(4)], axis=2).reshape(len(rows), 4 * rb)
    assert not codes[:, ns:].any(), "pad bits set"
    codes = codes[:, :ns]
    return tuple((codes == c).astype(np.uint8) for c in (CODE_HET, CODE_HOM, CODE_MISSING))


def bim_text(tsv_body):
    """one line per TSV row: chrom, locus (the dosage file's "chrom:pos:ref:alt"), 0, pos, alt, ref -- the TSV's columns"""
    out = []
    for row in tsv_body.split(b"\n"):
        if not row:
            continue
        f = row.split(b"\t")
        chrom, pos, ref, alt = f[0], f[1], f[3], f[4]
        out.append(b"\t".join([chrom, b":".join([chrom, pos, ref, alt]), b"0", pos, alt, ref]) + b"\n")
    return b"".join(out)


def normalized(names):
    """the names as --sample writes them (parse.NormalizeHeader: '.' -> '_')"""
    return [nm.replace(".", "_") for nm in names]


def fam_text(names):
    return "".join("%s\t%s\t0\t0\t0\t-9\n" % (nm, nm) for nm in normalized(names)).encode()


def expected_from_body(tsv_body, names, cfg=None):
    """{"bed", "bim", "fam"} of a TSV body (no header line) over the header's sample names"""
    names = normalized(names)
    if names:
        mats = pt.matrices(tsv_body, names, cfg)
        bed, bim = bed_bytes(*mats), bim_text(tsv_body)
    else:  # a file without sample columns: no rows
        bed, bim = MAGIC, b""
    return {"bed": bed, "bim": bim, "fam": fam_text(names)}


def expected(oracle_run, vcf, cfg=None):
    """(files, TSV body, log) of a VCF through the oracle (oracle_run: oracle_lib.run)"""
    rc, body, log, _ = oracle_run(vcf, cfg)
    assert rc == 0
    return expected_from_body(body, pt.sample_names(vcf), cfg), body, log


def read_files(prefix):
    out = {}
    for ext in ("bed", "bim", "fam"):
        with open("%s.%s" % (prefix, ext), "rb") as f:
            out[ext] = f.read()
    return out


def diff(got, want):
    """'' when the three files are equal, else where the first of them differs"""
    for ext in ("fam", "bim", "bed"):
        g, w = got[ext], want[ext]
        if g == w:
            continue
        n = min(len(g), len(w))
        at = next((i for i in range(n) if g[i] != w[i]), n)
        return ".%s: %d vs %d bytes, first difference at byte %d: got %r want %r" % (ext, len(g), len(w), at, g[at:at + 24], w[at:at + 24])
    return ""


# ---- maps for the exported per-row function

def dense_map(classes, pad_bits=0):
    """the library's dense class map of one row: 2 bits per sample, padded to 16 bytes; pad_bits: a value repeated into
    the 2-bit slots of samples >= S (the row must not depend on them)"""
    ns = len(classes)
    stride = max(16, (row_bytes(ns) + 15) // 16 * 16)
    full = np.full(4 * stride, pad_bits & 3, dtype=np.uint8)
    full[:ns] = classes
    q = full.reshape(stride, 4)
    return (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8).tobytes()


def short_list(entries):
    """BVCF_ALLELE_CMAP_SPARSE: uint32 n, then n entries (map byte index << 8 | map byte), ascending; 64 bytes"""
    words = [len(entries)] + [(idx << 8) | byte for idx, byte in sorted(entries)]
    words += [0] * (16 - len(words))
    return np.array(words, dtype="<u4").tobytes()


def row_of_classes(classes):
    """the expected .bed row of one row's classes (BVCF_CLS_* numbers)"""
    codes = np.array([[CLASS_TO_CODE[int(c)] for c in classes]], dtype=np.uint8)
    return pack_codes(codes)[0].tobytes()


# ---- inputs

ALIGN_SAMPLES = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 129, 299, 300]  # row_bytes 1 .. 75, odd ones among them
GPU_SAMPLE_COUNTS = sorted(set(ALIGN_SAMPLES) | {f[2] for f in pt.FUZZ if f[0] != 13} | set(pt.RARE_SAMPLES) | {70, 298, 8, 2504})


def align_vcf(ns):
    """the input of the alignment case at S = ns: the tiny_vcf shape for a handful of samples, rare_vcf's mix of short
    lists and dense maps above"""
    return pt.tiny_vcf(ns, n_lines=40) if ns < 16 else pt.rare_vcf(ns, n_lines=200, seed=7800 + ns)


def many_alts_vcf(ns=8, n_lines=1000, ref_len=67, seed=8700):
    """lines that emit ~200 ALT alleles each at 8 samples: three MNP ALTs that differ from a 67-base REF at every
    position give 201 rows of 2 bytes from some 340 bytes of text -- more than the quarter of the text the arena of the
    rows starts with"""
    rng = random.Random(seed)
    bases = "ACGT"
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        ref = "".join(rng.choice(bases) for _ in range(ref_len))
        alts = ["".join(bases[(bases.index(b) + 1 + j) % 4] for b in ref) for j in range(3)]
        gts = ["./." if rng.random() < 0.1 else "%d/%d" % (rng.randint(0, 3), rng.randint(0, 3)) for _ in range(ns)]
        out.append("\t".join(["chr4", str(1000 + 100 * k), ".", ref, ",".join(alts), "50", "PASS", ".", "GT"] + gts) + "\n")
    return "".join(out).encode()


FUZZ_SEEDS = [11, 12, 14]  # pairtable.FUZZ without seed 13, whose rows all have dozens of carriers (no short list to expand)
MASKED = "fuzz70crlf"      # the gtmask input of the composition case (GT:DP:GQ, CRLF, rare lines behind the cohort's)


def seeded_inputs():
    """every seeded (not crafted) input of the GPU cases: {name: bytes}"""
    import gtmask
    d = {"fuzz%d" % s: pt.fuzz_vcf(s) for s in FUZZ_SEEDS}
    d.update({"rare%d" % ns: pt.rare_vcf(ns) for ns in pt.RARE_SAMPLES})
    d.update({"align%d" % ns: align_vcf(ns) for ns in ALIGN_SAMPLES if ns >= 16})
    d[MASKED] = gtmask.seeded(MASKED)
    return d
