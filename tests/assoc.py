"""--pheno / --assoc: the expected records and both output files, written from the rules of include/bvcf.h alone and built
from the oracle's TSV of the same bytes.

A value is the exact rational its text denotes (fractions.Fraction); Y is the integer nearest to y 10^6, ties away from
zero, |y| <= 10^6.  A row's heterozygotes / homozygotes / missingGenos lists give the classes; the sums are Python integers;
float(int) is the correctly rounded double; the statistic is the sequence of include/bvcf.h operation for operation, with
erfc taken from the same libm through ctypes (math.erfc is CPython's own).  Test infrastructure only."""
import ctypes
import ctypes.util
import math
import random
import re
from fractions import Fraction

import numpy as np

import pairtable as pt
import variantlist as vl
import vcfgen

ONE = 10 ** 6
MAX_Y = 10 ** 12
MAX_COLUMNS = 16
MAX_TEXT = 64
MAX_SAMPLES = 1 << 22
VALUE_RE = re.compile(rb"[+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]{1,3})?")
HEADER = "chrom\tpos\tref\talt\tpheno\tn\taltFreq\tbeta\tse\tchisq\tp"

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.erfc.restype = ctypes.c_double
_libm.erfc.argtypes = [ctypes.c_double]


def erfc(x):
    return _libm.erfc(x)


class PhenoFileError(Exception):
    def __init__(self, line, what):
        super().__init__("line %d: %s" % (line, what) if line else what)
        self.line = line


def value(text):
    """Y of a value's text (bytes); ValueError for text outside the grammar, OverflowError for |y| > 10^6"""
    if len(text) > MAX_TEXT or not VALUE_RE.fullmatch(text):
        raise ValueError(text)
    m = re.fullmatch(rb"([+-]?)([0-9]*)\.?([0-9]*)(?:[eE]([+-]?[0-9]+))?", text)
    sign, ip, fp, ex = m.groups()
    y = Fraction(int((ip + fp) or b"0"), 10 ** len(fp)) * Fraction(10) ** int(ex or b"0")
    if y > ONE:
        raise OverflowError(text)
    x = y * ONE
    n = (2 * x.numerator + x.denominator) // (2 * x.denominator)  # floor(x + 1/2): ties up, x >= 0
    return -n if sign == b"-" else n


def limbs(v, n=16):
    """v as n balanced base-256 digits, least significant first"""
    out = []
    for _ in range(n):
        d = ((v + 128) & 255) - 128
        out.append(d)
        v = (v - d) >> 8
    assert v == 0
    return out


def n_limbs(v):
    return max([1] + [a + 1 for a, d in enumerate(limbs(v)) if d])


def parse_file(text, sample_names):
    """(names, Y [K][S] integers, P [K][S] flags, samples named) of a phenotype file against the (kept) sample names;
    PhenoFileError names the line"""
    cols = {}
    for i, nm in enumerate(sample_names):
        cols.setdefault(nm.encode() if isinstance(nm, str) else nm, []).append(i)
    names, k, seen, rows = None, None, {}, []
    for no, ln in enumerate(text.split(b"\n"), 1):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln:
            continue
        f = ln.split(b"\t")
        if ln.startswith(b"#") and k is not None:
            raise PhenoFileError(no, "a # line behind the first")
        if k is None:
            k = len(f) - 1
            if not 1 <= k <= MAX_COLUMNS:
                raise PhenoFileError(no, "columns")
            if ln.startswith(b"#"):
                if f[0] != b"#sample" or any(not x for x in f[1:]) or len(set(f[1:])) != k:
                    raise PhenoFileError(no, "header")
                names = f[1:]
                continue
            names = [b"PHENO%d" % (i + 1) for i in range(k)]
        if len(f) != k + 1:
            raise PhenoFileError(no, "field count")
        if not f[0]:
            raise PhenoFileError(no, "empty name")
        try:
            vals = [None if x == b"NA" else value(x) for x in f[1:]]
        except (ValueError, OverflowError):
            raise PhenoFileError(no, "bad value")
        if f[0] not in cols:
            continue
        if len(cols[f[0]]) > 1:
            raise PhenoFileError(no, "ambiguous name")
        if f[0] in seen:
            raise PhenoFileError(no, "sample twice")
        seen[f[0]] = no
        rows.append((cols[f[0]][0], vals))
    if k is None:
        raise PhenoFileError(0, "no line")
    S = len(sample_names)
    Y = [[0] * S for _ in range(k)]
    P = [[0] * S for _ in range(k)]
    for i, vals in rows:
        for c, v in enumerate(vals):
            if v is not None:
                Y[c][i], P[c][i] = v, 1
    return names, Y, P, len(rows)


def decimal(y):
    """Y / 10^6 as exact text"""
    s = "-" if y < 0 else ""
    q, r = divmod(abs(y), ONE)
    s += str(q)
    if r:
        s += "." + ("%06d" % r).rstrip("0")
    return s


def file_text(rows, names=None, eol=b"\n"):
    """a phenotype file of [(sample name, [value texts, integers Y or None for NA])]"""
    out = []
    if names is not None:
        out.append(b"\t".join([b"#sample"] + list(names)))
    for nm, vs in rows:
        out.append(b"\t".join([nm] + [b"NA" if x is None else x if isinstance(x, bytes) else decimal(x).encode() for x in vs]))
    return b"".join(x + eol for x in out)


def totals(Y, P):
    """[(NP, AY, BY)] per column"""
    return [(sum(p), sum(y), sum(v * v for v in y)) for y, p in zip(Y, P)]


def records(H, O, M, Y, P):
    """[rows][K] tuples (N_het, N_hom, N_mis, A_het, A_hom, A_mis, B_mis) of class matrices [rows][S] (exact: the sums stay
    far below 2^63 per 21-bit piece, Python integers put the pieces together)"""
    n_rows, S = H.shape
    K = len(Y)
    out = [[None] * K for _ in range(n_rows)]
    cls = [x.astype(np.int64) for x in (H, O, M)]
    for k in range(K):
        p = np.array(P[k], dtype=np.int64)
        cnt = [(c @ p).tolist() if S else [0] * n_rows for c in cls]
        sums = []
        for c, vec in list(zip(cls, [Y[k]] * 3)) + [(cls[2], [v * v for v in Y[k]])]:
            tot = [0] * n_rows
            for j in range(4):  # |v| < 2^84 in four 21-bit pieces: every int64 product is exact
                piece = np.array([(1 if v >= 0 else -1) * ((abs(v) >> (21 * j)) & ((1 << 21) - 1)) for v in vec], dtype=np.int64)
                part = (c @ piece).tolist() if S else [0] * n_rows
                tot = [t + (x << (21 * j)) for t, x in zip(tot, part)]
            sums.append(tot)
        for r in range(n_rows):
            out[r][k] = (cnt[0][r], cnt[1][r], cnt[2][r], sums[0][r], sums[1][r], sums[2][r], sums[3][r])
    return out


def ints(rec, tot):
    """(n, Sg, c, va, vb) of a record against its column's totals"""
    n_het, n_hom, n_mis, a_het, a_hom, a_mis, b_mis = rec
    NP, AY, BY = tot
    n = NP - n_mis
    sy = AY - a_mis
    syy = BY - b_mis
    sg = n_het + 2 * n_hom
    sgg = n_het + 4 * n_hom
    sgy = a_het + 2 * a_hom
    return n, sg, n * sgy - sg * sy, n * sgg - sg * sg, n * syy - sy * sy


def stat(rec, tot):
    """(n, altFreq or None, (beta, se, chisq, p) or None): the sequence of include/bvcf.h, operation for operation"""
    n, sg, c, va, vb = ints(rec, tot)
    freq = float(sg) / float(2 * n) if n > 0 else None
    if n < 3 or va == 0 or vb == 0:
        return n, freq, None
    dc, dva, dvb = float(c), float(va), float(vb)
    r2 = min(1.0, (dc / dva) * (dc / dvb))
    chisq = float(n) * r2
    beta = dc / dva / 1e6
    se = math.sqrt((dvb / dva) * (1.0 - r2) / float(n - 2)) / 1e6
    p = erfc(math.sqrt(chisq / 2.0))
    return n, freq, (beta, se, chisq, p)


def g3(x):
    return "0" if x == 0 else "%.3G" % x


def output_text(recs, tots, loci_cols, names, empty="!"):
    """the --assoc file: loci_cols[r] = the row's four TSV columns (str)"""
    out = [HEADER]
    tested = 0
    for r, row in enumerate(recs):
        for k, rec in enumerate(row):
            n, freq, st = stat(rec, tots[k])
            f = list(loci_cols[r]) + [names[k].decode(), str(n), empty if freq is None else g3(freq)]
            f += [empty] * 4 if st is None else [g3(x) for x in st]
            tested += st is not None
            out.append("\t".join(f))
    return ("\n".join(out) + "\n").encode(), tested


def report_text(k, n_named, rows, tested):
    return ("columns\t%d\nsamples\t%d\nrows\t%d\ntested\t%d\n" % (k, n_named, rows, tested)).encode()


def loci_columns(tsv_body):
    return [tuple(f[c].decode() for c in vl.COLS) for f in (row.split(b"\t") for row in vl.rows_of(tsv_body))]


def expected_m(H, O, M, loci_cols, sample_names, pheno_text, empty="!"):
    """(records, totals, output file, report file) of class matrices"""
    names, Y, P, n_named = parse_file(pheno_text, sample_names)
    recs = records(H, O, M, Y, P)
    tots = totals(Y, P)
    text, tested = output_text(recs, tots, loci_cols, names, empty)
    return recs, tots, text, report_text(len(names), n_named, len(recs), tested)


def expected(oracle_run, vcf, pheno_text, cfg=None):
    """(records, totals, output file, report file, TSV body, log) of a VCF through the oracle"""
    cfg = cfg or {}
    rc, body, log, _ = oracle_run(vcf, cfg)
    assert rc == 0
    sn = pt.sample_names(vcf)
    if not sn:
        names = parse_file(pheno_text, [])[0]
        return [], [], (HEADER + "\n").encode(), report_text(len(names), 0, 0, 0), body, log
    H, O, M = pt.matrices(body, sn, cfg)
    return expected_m(H, O, M, loci_columns(body), sn, pheno_text, cfg.get("emptyField", "!")) + (body, log)


# ---- inputs

def mixed_rows(sample_names, k, seed, big=False, na=0.1, absent=0.05, binary_column=None, extra=(b"NOBODY", b"nobody2")):
    """a file's rows over the samples: K columns of mixed sign and magnitude (big: +-10^12 beside small ones), some NA, some
    samples not named at all, and names no sample has"""
    rng = random.Random(seed)
    rows = []
    sample_names = [x.encode() if isinstance(x, str) else x for x in sample_names]
    for nm in list(sample_names) + list(extra):
        if nm in sample_names and rng.random() < absent:
            continue
        vs = []
        for c in range(k):
            u = rng.random()
            if u < na:
                vs.append(None)
            elif c == binary_column:
                vs.append(rng.choice([0, ONE]))
            elif big and u < 0.3:
                vs.append(rng.choice([MAX_Y, -MAX_Y, MAX_Y - 1, 1 - MAX_Y]))
            elif big:
                vs.append(rng.randint(-MAX_Y, MAX_Y))
            else:
                vs.append(rng.randint(-100 * (c + 1), 100 * (c + 1)))
        rows.append((nm, vs))
    rng.shuffle(rows)
    return rows


def pheno_for(vcf, k, seed, names=None, **kw):
    return file_text(mixed_rows(pt.sample_names(vcf), k, seed, **kw), names)


DENSE_ROWS = [1, 15, 16, 17, 63, 64, 65, 130]


def dense_vcf(n_rows, ns=70, seed=4000):
    """n_rows rows with carriers in more than 15 map bytes each (dense maps), every row different, and one sparse row"""
    rng = random.Random(seed + n_rows)
    out = [vcfgen.header(ns)]
    for r in range(n_rows):
        gts = [rng.choice(["0|1", "1|1", "0|0", "./.", "1|0"]) for _ in range(ns)]
        for s in range(0, ns, 4):  # a carrier in every map byte
            gts[s] = rng.choice(["0|1", "1|1"])
        out.append(pt.snp_line(100 + 10 * r, gts))
    out.append(pt.snp_line(100 + 10 * n_rows, ["0|1"] + ["0|0"] * (ns - 1)))
    return "".join(out).encode()


def special_vcf(ns=24):
    """an all-hom row (va = 0), a row in which every sample is missing, a row with two called samples (n = 2), haploid calls,
    a sample missing in every row (the last)"""
    m = ["./."]
    out = [vcfgen.header(ns),
           pt.snp_line(100, ["1|1"] * (ns - 1) + m),
           pt.snp_line(200, ["0|1"] + ["./."] * (ns - 1)),
           pt.snp_line(300, ["0|1", "1|1"] + ["./."] * (ns - 2)),
           pt.snp_line(400, ["1", "0", "1", "."] * ((ns - 1) // 4) + ["0|1"] * ((ns - 1) % 4) + m),
           pt.snp_line(500, ["0|1", "0|0", "1|1"] * ((ns - 1) // 3) + ["0|0"] * ((ns - 1) % 3) + m)]
    return "".join(out).encode()


def many_alts_vcf(ns=20, n_lines=400):
    """three ALTs a line: three rows from some 110 bytes of text"""
    rng = random.Random(4100)
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        gts = ["%d|%d" % (rng.randint(0, 3), rng.randint(0, 3)) for _ in range(ns)]
        out.append("\t".join(["chr7", str(100 + 3 * k), ".", "A", "C,G,T", "50", "PASS", ".", "GT"] + gts) + "\n")
    return "".join(out).encode()


def big_missing_vcf(ns=300):
    """300 samples all missing in one row beside carriers in another: with Y = 10^12, B_mis = 3 * 10^26 passes 2^64"""
    out = [vcfgen.header(ns), pt.snp_line(100, ["./."] * (ns - 1) + ["0|1"]), pt.snp_line(200, ["0|1", "1|1", "./.", "0|0"] * (ns // 4))]
    return "".join(out).encode()
