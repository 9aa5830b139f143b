"""--score: the expected per-sample scores and both output files, written from the rules of include/bvcf.h alone and built
from the oracle's TSV of the same bytes.

A weight is the exact rational its text denotes (fractions.Fraction); W is the integer nearest to w 10^12, ties away from
zero, |W| <= 10^18.  A row of the TSV is matched when its locus "chrom:pos:ref:alt" is an entry of the score file; its
heterozygotes / homozygotes / missingGenos lists give the dosages 1 / 2 / missing.  T = sum W g in Python integers.  Test
infrastructure only."""
import random
import re
from fractions import Fraction

import numpy as np

import pairtable as pt
import variantlist as vl
import vcfgen

ONE = 10 ** 12
MAX_W = 10 ** 18
MAX_COLUMNS = 64
MAX_TEXT = 64
WEIGHT_RE = re.compile(rb"[+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]{1,3})?")


class ScoreFileError(Exception):
    def __init__(self, line, what):
        super().__init__("line %d: %s" % (line, what) if line else what)
        self.line = line


def weight(text):
    """W of a weight's text (bytes); ValueError for text outside the grammar, OverflowError for |W| > 10^18"""
    if len(text) > MAX_TEXT or not WEIGHT_RE.fullmatch(text):
        raise ValueError(text)
    m = re.fullmatch(rb"([+-]?)([0-9]*)\.?([0-9]*)(?:[eE]([+-]?[0-9]+))?", text)
    sign, ip, fp, ex = m.groups()
    w = Fraction(int((ip + fp) or b"0"), 10 ** len(fp)) * Fraction(10) ** int(ex or b"0")
    x = w * ONE
    n = (2 * x.numerator + x.denominator) // (2 * x.denominator)  # floor(x + 1/2): ties up, x >= 0
    if n > MAX_W:
        raise OverflowError(text)
    return -n if sign == b"-" else n


def limbs(w, n=8):
    """W as n balanced base-256 digits, least significant first"""
    out = []
    for _ in range(n):
        d = ((w + 128) & 255) - 128
        out.append(d)
        w = (w - d) >> 8
    assert w == 0
    return out


def n_limbs(w):
    ls = limbs(w)
    return max([1] + [a + 1 for a, d in enumerate(ls) if d])


def decimal(t):
    """T / 10^12 as exact text"""
    s = "-" if t < 0 else ""
    q, r = divmod(abs(t), ONE)
    s += str(q)
    if r:
        s += "." + ("%012d" % r).rstrip("0")
    return s


def parse_file(text):
    """(names, [(locus, [W_k])]) of a score file by its rules; ScoreFileError names the line"""
    names, entries, seen, k = None, [], {}, None
    for no, ln in enumerate(text.split(b"\n"), 1):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln:
            continue
        f = ln.split(b"\t")
        if ln.startswith(b"#") and k is not None:
            raise ScoreFileError(no, "a # line behind the first")
        if k is None:
            k = len(f) - 1
            if not 1 <= k <= MAX_COLUMNS:
                raise ScoreFileError(no, "columns")
            if ln.startswith(b"#"):
                if f[0] != b"#locus" or any(not x for x in f[1:]) or len(set(f[1:])) != k:
                    raise ScoreFileError(no, "header")
                names = f[1:]
                continue
            names = [b"SCORE%d" % (i + 1) for i in range(k)]
        if len(f) != k + 1:
            raise ScoreFileError(no, "field count")
        if not f[0]:
            raise ScoreFileError(no, "empty locus")
        if f[0] in seen:
            raise ScoreFileError(no, "locus twice")
        seen[f[0]] = no
        try:
            ws = [weight(x) for x in f[1:]]
        except (ValueError, OverflowError):
            raise ScoreFileError(no, "bad weight")
        entries.append((f[0], ws))
    if k is None:
        raise ScoreFileError(0, "no line")
    return names, entries


def file_text(entries, names=None, eol=b"\n", fmt=None):
    """a score file of [(locus, [weight texts or integers W])]: an integer W is written as the decimal of W / 10^12"""
    out = []
    if names is not None:
        out.append(b"\t".join([b"#locus"] + list(names)))
    for loc, ws in entries:
        out.append(b"\t".join([loc] + [x if isinstance(x, bytes) else decimal(x).encode() for x in ws]))
    return b"".join(x + eol for x in out)


def sums_m(H, O, M, loci, entries, k):
    """(T [S][K] Python integers, G [S], X [S], R) of dosage matrices whose rows have the given loci.  |W| < 2^63 is cut into
    three signed 21-bit pieces, so that every int64 matrix product is exact; Python integers put them together"""
    table = dict(entries)
    idx = [r for r, loc in enumerate(loci) if loc in table]
    ns = H.shape[1]
    g = H[idx].astype(np.int64) + 2 * O[idx].astype(np.int64)
    G = g.sum(axis=0)
    X = M[idx].astype(np.int64).sum(axis=0)
    T = [[0] * k for _ in range(ns)]
    assert len(idx) < 1 << 40
    if idx:
        W = [table[loci[r]] for r in idx]
        for j in range(3):
            P = np.array([[(1 if w >= 0 else -1) * ((abs(w) >> (21 * j)) & ((1 << 21) - 1)) for w in row] for row in W], dtype=np.int64)
            part = (g.T @ P).tolist()
            for i in range(ns):
                Ti, pi = T[i], part[i]
                for c in range(k):
                    Ti[c] += pi[c] << (21 * j)
    return T, G.tolist(), X.tolist(), len(idx)


def sums(tsv_body, sample_names, entries, k, cfg=None):
    """the same of a TSV body"""
    H, O, M = pt.matrices(tsv_body, sample_names, cfg)
    return sums_m(H, O, M, vl.loci_of(tsv_body), entries, k)


def output_text(T, G, X, R, sample_names, names, empty="!"):
    out = ["\t".join(["sample", "matched", "called", "dosageSum"] + [x for nm in names for x in (nm.decode() + "_SUM", nm.decode() + "_AVG")])]
    for i, nm in enumerate(sample_names):
        called = R - X[i]
        f = [nm, str(R), str(called), str(G[i])]
        for t in T[i]:
            f.append(decimal(t))
            if not called:
                f.append(empty)
            elif t == 0:
                f.append("0")
            else:
                f.append("%.6G" % (float(t) / float(ONE * 2 * called)))  # (int -> float and float / float round correctly)
        out.append("\t".join(f))
    return ("\n".join(out) + "\n").encode()


def report_text(n_listed, k, R):
    return ("listed\t%d\ncolumns\t%d\nmatchedRows\t%d\n" % (n_listed, k, R)).encode()


def expected(oracle_run, vcf, score_text, cfg=None):
    """((T, G, X, R), output file, report file, TSV body, log) of a VCF through the oracle"""
    cfg = cfg or {}
    rc, body, log, _ = oracle_run(vcf, cfg)
    assert rc == 0
    names, entries = parse_file(score_text)
    sn = pt.sample_names(vcf)
    t = sums(body, sn, entries, len(names), cfg) if sn else ([], [], [], 0)
    return (t, output_text(*t, sn, names, cfg.get("emptyField", "!")), report_text(len(entries), len(names), t[3]), body, log)


# ---- inputs

def mixed_weights(rng, k, big=False):
    """K integer weights of mixed sign and size; big: +-10^18 beside +-1 (eight limbs)"""
    out = []
    for c in range(k):
        kind = rng.random()
        if big and kind < 0.3:
            w = rng.choice([MAX_W, -MAX_W, MAX_W - 1, 1 - MAX_W])
        elif big and kind < 0.5:
            w = rng.choice([1, -1])
        elif big:
            w = rng.randint(-MAX_W, MAX_W)
        else:
            w = rng.randint(-127, 127)
        out.append(w)
    return out


def entries_for(loci, k, seed, big=False, frac=1.0, zero_column=None, extra=()):
    """entries over a seeded fraction of the loci (deduplicated, in order), plus loci that match nothing; zero_column: a
    column whose weights all quantise to 0 (given as text)"""
    rng = random.Random(seed)
    seen, out = set(), []
    for loc in list(loci) + list(extra):
        if loc in seen or (loc not in extra and rng.random() >= frac):
            continue
        seen.add(loc)
        ws = mixed_weights(rng, k, big)
        if not any(ws):
            ws[0] = 1
        if zero_column is not None:
            ws[zero_column] = rng.choice([b"0", b"4.9999e-13", b"-0.0000000000004", b"0e5", b"-.0"])
        out.append((loc, ws))
    return out


COLUMN_EDGES = [1, 15, 16, 17, 64]
FLUSH_ROWS = 150000


def flush_vcf(ns=8):
    """FLUSH_ROWS identical all-hom rows (distinct positions would need as many entries: the same line, one entry)"""
    line = pt.snp_line(100, ["1|1"] * ns)
    return (vcfgen.header(ns) + line * FLUSH_ROWS).encode()


def multiallelic_vcf(ns=20):
    rng = random.Random(9100)
    out = [vcfgen.header(ns)]
    for k in range(30):
        gts = [rng.choice(["0|0", "0|1", "1|2", "2|2", "./.", "1|1", "0|2", "2"]) for _ in range(ns)]
        out.append("\t".join(["chr5", str(100 + 7 * k), ".", "A", "C,G", "50", "PASS", ".", "GT"] + gts) + "\n")
    return "".join(out).encode()


def all_hom_vcf(ns=10):
    out = [vcfgen.header(ns), pt.snp_line(100, ["1|1"] * ns), pt.snp_line(200, ["1/1"] * (ns - 1) + ["./."]),
           pt.snp_line(300, ["0|1"] * ns), pt.snp_line(400, ["1"] * ns)]
    return "".join(out).encode()


def twice_vcf(ns=6):
    """one locus on two lines: both match"""
    rng = random.Random(9200)
    out = [vcfgen.header(ns)]
    for pos in (100, 100, 150, 100):
        out.append(pt.snp_line(pos, [rng.choice(["0|1", "1|1", "0|0", "./."]) for _ in range(ns - 1)] + ["0|1"]))
    return "".join(out).encode()
