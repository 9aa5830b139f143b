"""--covar: the expected records and both output files of the covariate-adjusted scan, written from the rules of
include/bvcf.h alone and built from the oracle's TSV of the same bytes.

Values are exact rationals (assoc.value: fractions.Fraction); a row's heterozygotes / homozygotes / missingGenos lists give
the classes; every sum is a Python integer; float(int) is the correctly rounded double; the LDL^T and the statistic follow
include/bvcf.h operation for operation in Python floats, with erfc from the same libm through ctypes (assoc.erfc).  The Gram
matrix is summed straight from its definition over the sample set (gram); gram_of_records puts it together from the records
and the totals as the library does, and the tests hold the two against each other.  Test infrastructure only."""
import math
import random

import numpy as np

import assoc
import pairtable as pt

MAX_COVARS = 16
TINY = 2.0 ** -30

# The model's beta and se against numpy.linalg.lstsq on the called samples of well-conditioned random data
# (test_assoc_cov_cpu.py::test_model_against_lstsq, seeds LSTSQ_SEEDS): the largest relative deviation measured there, on the
# CPU, and the bound the test asserts -- eight times that value, the rule of tests/pca.py.  Never taken from the device.
LSTSQ_SEEDS = list(range(9100, 9112))
LSTSQ_MEASURED = 1.109e-14
LSTSQ_BOUND = 8 * LSTSQ_MEASURED


class CovarFileError(Exception):
    def __init__(self, line, what):
        super().__init__("line %d: %s" % (line, what) if line else what)
        self.line = line


def parse_file(text, sample_names):
    """(names, C [J][S] integers, complete [S] flags, samples named) of a covariate file against the (kept) sample names"""
    cols = {}
    for i, nm in enumerate(sample_names):
        cols.setdefault(nm.encode() if isinstance(nm, str) else nm, []).append(i)
    names, j, lead, seen, rows = None, None, 1, {}, []
    for no, ln in enumerate(text.split(b"\n"), 1):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln:
            continue
        f = ln.split(b"\t")
        if ln.startswith(b"#") and j is not None:
            raise CovarFileError(no, "a # line behind the first")
        if j is None:
            if ln.startswith(b"#") and f[:2] == [b"#FID", b"IID"]:
                lead = 2
            j = len(f) - lead
            if not 1 <= j <= MAX_COVARS:
                raise CovarFileError(no, "covariates")
            if ln.startswith(b"#"):
                if (lead == 1 and f[0] != b"#sample") or any(not x for x in f[lead:]) or len(set(f[lead:])) != j:
                    raise CovarFileError(no, "header")
                names = f[lead:]
                continue
            names = [b"COV%d" % (i + 1) for i in range(j)]
        if len(f) != j + lead:
            raise CovarFileError(no, "field count")
        name = f[lead - 1]
        if not name:
            raise CovarFileError(no, "empty name")
        try:
            vals = [None if x == b"NA" else assoc.value(x) for x in f[lead:]]
        except (ValueError, OverflowError):
            raise CovarFileError(no, "bad value")
        if name not in cols:
            continue
        if len(cols[name]) > 1:
            raise CovarFileError(no, "ambiguous name")
        if name in seen:
            raise CovarFileError(no, "sample twice")
        seen[name] = no
        rows.append((cols[name][0], vals))
    if j is None:
        raise CovarFileError(0, "no line")
    S = len(sample_names)
    Cv = [[0] * S for _ in range(j)]
    complete = [0] * S
    for i, vals in rows:
        if all(v is not None for v in vals):
            complete[i] = 1
            for q, v in enumerate(vals):
                Cv[q][i] = v
    return names, Cv, complete, len(rows)


def file_text(rows, names=None, eol=b"\n", fid=False):
    """a covariate file of [(sample name, [value texts, integers C or None for NA])]; fid: the "#FID IID" form"""
    out = []
    if fid:
        out.append(b"\t".join([b"#FID", b"IID"] + list(names)))
    elif names is not None:
        out.append(b"\t".join([b"#sample"] + list(names)))
    for nm, vs in rows:
        f = [b"NA" if x is None else x if isinstance(x, bytes) else assoc.decimal(x).encode() for x in vs]
        out.append(b"\t".join(([b"fam", nm] if fid else [nm]) + f))
    return b"".join(x + eol for x in out)


def mask(Y, P, complete):
    """the phenotypes of the incomplete samples go"""
    Pm = [[p and c for p, c in zip(row, complete)] for row in P]
    Ym = [[y if p else 0 for y, p in zip(yr, pr)] for yr, pr in zip(Y, Pm)]
    return Ym, Pm


def groups(P):
    """(group of every phenotype, the groups' first phenotypes): the same presence vector, the same group"""
    first, group_of = [], []
    for k, row in enumerate(P):
        for g, f in enumerate(first):
            if P[f] == row:
                group_of.append(g)
                break
        else:
            group_of.append(len(first))
            first.append(k)
    return group_of, first


class Layout:
    """where a covariate record's words and operand B's columns are (include/bvcf.h)"""

    def __init__(self, J, K, G, lc, lcc, lcy):
        self.J, self.K, self.G, self.lc, self.lcc, self.lcy = J, K, G, lc, lcc, lcy
        self.np2 = J * (J + 1) // 2
        self.gw = 3 * J + 2 * self.np2
        self.w = G * self.gw + K * 2 * J
        self.vc, self.vcc, self.vcy = 16 // lc, 16 // lcc, 16 // lcy
        self.nc, self.ncc, self.ncy = G * J, G * self.np2, K * J
        self.bc, self.bcc, self.bcy = (-(-n // v) for n, v in ((self.nc, self.vc), (self.ncc, self.vcc), (self.ncy, self.vcy)))
        self.n_blocks = self.bc + self.bcc + self.bcy

    def word_c(self, g, cls, j):
        return g * self.gw + cls * self.J + j

    def word_cc(self, g, i, j):
        return g * self.gw + 3 * self.J + 2 * (j * (j + 1) // 2 + i)

    def word_cy(self, k, j):
        return self.G * self.gw + 2 * self.J * k + 2 * j

    def col_c(self, g, j):
        v = g * self.J + j
        return 16 * (v // self.vc) + (v % self.vc) * self.lc

    def col_cc(self, g, i, j):
        v = g * self.np2 + j * (j + 1) // 2 + i
        return 16 * (self.bc + v // self.vcc) + (v % self.vcc) * self.lcc

    def col_cy(self, k, j):
        v = k * self.J + j
        return 16 * (self.bc + self.bcc + v // self.vcy) + (v % self.vcy) * self.lcy


def layout_of(Cv, Y, P):
    """the layout of masked data: the smallest limb counts that hold the values a column can get"""
    J, K = len(Cv), len(Y)
    group_of, first = groups(P)
    anyone = [i for i in range(len(Cv[0]) if Cv else 0) if any(P[k][i] for k in range(K))]
    # (a complete sample without any phenotype still counts for the C and CC limbs: the table does not look at P there)
    lc = max([1] + [assoc.n_limbs(Cv[q][i]) for q in range(J) for i in range(len(Cv[q]))])
    lcc = max([1] + [assoc.n_limbs(Cv[p][i] * Cv[q][i]) for q in range(J) for p in range(q + 1) for i in range(len(Cv[q]))])
    lcy = max([1] + [assoc.n_limbs(Cv[q][i] * Y[k][i]) for q in range(J) for k in range(K) for i in anyone if P[k][i]])
    return Layout(J, K, len(first), lc, lcc, lcy), group_of, first


def _sums(cls, vec):
    """[rows] exact sums of vec (Python integers below 2^84 in size) over the samples of a class matrix [rows][S]"""
    n_rows, S = cls.shape
    if not S:
        return [0] * n_rows
    tot = [0] * n_rows
    for j in range(4):  # four 21-bit pieces: every int64 product is exact
        piece = np.array([(1 if v >= 0 else -1) * ((abs(v) >> (21 * j)) & ((1 << 21) - 1)) for v in vec], dtype=np.int64)
        if piece.any():
            tot = [t + (x << (21 * j)) for t, x in zip(tot, (cls @ piece).tolist())]
    return tot


def _u64(v):
    return v & ((1 << 64) - 1)


def cov_words(H, O, M, Cv, Y, P, lay, group_of, first):
    """[rows][W] the covariate records as unsigned 64-bit words (masked Y / P)"""
    n_rows = H.shape[0]
    out = [[0] * lay.w for _ in range(n_rows)]
    cls = [x.astype(np.int64) for x in (H, O, M)]

    def put(at, vals, wide):
        for r, v in enumerate(vals):
            out[r][at] = _u64(v)
            if wide:
                out[r][at + 1] = _u64(v >> 64)

    for g, f in enumerate(first):
        pg = P[f]
        for j in range(lay.J):
            cj = [c if p else 0 for c, p in zip(Cv[j], pg)]
            for c in range(3):
                put(lay.word_c(g, c, j), _sums(cls[c], cj), False)
            for i in range(j + 1):
                put(lay.word_cc(g, i, j), _sums(cls[2], [a * b if p else 0 for a, b, p in zip(Cv[i], Cv[j], pg)]), True)
    for k in range(lay.K):
        for j in range(lay.J):
            put(lay.word_cy(k, j), _sums(cls[2], [c * y if p else 0 for c, y, p in zip(Cv[j], Y[k], P[k])]), True)
    return out


def totals_row(Cv, Y, P, lay, group_of, first):
    """[W] the totals row: the sums over all samples in the missing-class places"""
    S = len(P[0]) if P else 0
    ones = np.ones((1, S), dtype=np.int64)
    zero = np.zeros((1, S), dtype=np.int64)
    return cov_words(zero, zero, ones, Cv, Y, P, lay, group_of, first)[0]


def _exact_gram(V):
    """V [m][n] Python integers -> the lower triangle of V V^T, exact"""
    m = len(V)
    n = len(V[0]) if m else 0
    top = max([1] + [abs(x) for row in V for x in row])
    A = np.array(V, dtype=np.int64 if top * top * max(n, 1) < 1 << 62 else object).reshape(m, n)
    G = A @ A.T
    return [[int(G[a][b]) for b in range(a + 1)] for a in range(m)]


def gram(h, o, m, Cv, y, p):
    """the Gram matrix (lower triangle, Python integers) of one row (class vectors h, o, m over the samples) and one phenotype
    (y, p), straight from the definition: v_0 = 1, v_1 .. v_J = C_j, v_{J+1} = g, v_{J+2} = Y over {P = 1 and called}"""
    idx = [i for i in range(len(p)) if p[i] and not m[i]]
    V = [[1] * len(idx)] + [[c[i] for i in idx] for c in Cv] + [[int(h[i]) + 2 * int(o[i]) for i in idx], [y[i] for i in idx]]
    return _exact_gram(V)


def _i64(w):
    return w - (1 << 64) if w >> 63 else w


def _i128(lo, hi):
    v = (hi << 64) | lo
    return v - (1 << 128) if v >> 127 else v


def gram_of_records(rec, tot, row, tot_row, lay, k, g):
    """the same matrix from a phenotype's record (assoc.records' tuple) and totals, the row's covariate words and the totals
    row: a total minus what was summed over the missing samples, or a sum over het / hom"""
    n_het, n_hom, n_mis, a_het, a_hom, a_mis, b_mis = rec
    NP, AY, BY = tot
    J = lay.J
    G = [[0] * (a + 1) for a in range(J + 3)]
    G[0][0] = NP - n_mis
    for j in range(J):
        G[1 + j][0] = _i64(tot_row[lay.word_c(g, 2, j)]) - _i64(row[lay.word_c(g, 2, j)])
        G[J + 1][1 + j] = _i64(row[lay.word_c(g, 0, j)]) + 2 * _i64(row[lay.word_c(g, 1, j)])
        for i in range(j + 1):
            at = lay.word_cc(g, i, j)
            G[1 + j][1 + i] = _i128(tot_row[at], tot_row[at + 1]) - _i128(row[at], row[at + 1])
        at = lay.word_cy(k, j)
        G[J + 2][1 + j] = _i128(tot_row[at], tot_row[at + 1]) - _i128(row[at], row[at + 1])
    G[J + 1][0] = n_het + 2 * n_hom
    G[J + 1][J + 1] = n_het + 4 * n_hom
    G[J + 2][0] = AY - a_mis
    G[J + 2][J + 1] = a_het + 2 * a_hom
    G[J + 2][J + 2] = BY - b_mis
    return G


def stat(G, J):
    """(n, altFreq or None, (beta, se, chisq, p) or None, collinear): the sequence of include/bvcf.h, operation for operation"""
    n, sg = G[0][0], G[J + 1][0]
    freq = float(sg) / float(2 * n) if n > 0 else None
    if n < J + 3:
        return n, freq, None, False
    m = J + 3
    D = [[float(G[a][b]) for b in range(a + 1)] for a in range(m)]
    u = [[0.0] * m for _ in range(m)]
    L = [[0.0] * m for _ in range(m)]
    d = [0.0] * m
    rss0 = 0.0
    for a in range(m):
        for b in range(a):
            s = D[a][b]
            for t in range(b):
                s = s - u[a][t] * L[b][t]
            u[a][b] = s
            L[a][b] = s / d[b]
        s = D[a][a]
        for t in range(a):
            s = s - u[a][t] * L[a][t]
            if a == J + 2 and t == J:
                rss0 = s
        d[a] = s
        if a <= J + 1 and not d[a] > D[a][a] * TINY:
            return n, freq, None, a <= J
    if not rss0 > D[J + 2][J + 2] * TINY:
        return n, freq, None, False
    bg, ug = L[J + 2][J + 1], u[J + 2][J + 1]
    r2 = (ug * bg) / rss0
    if not r2 < 1.0:
        r2 = 1.0
    if not r2 > 0.0:
        r2 = 0.0
    chisq = float(n) * r2
    beta = bg / 1e6
    se = math.sqrt((rss0 / d[J + 1]) * (1.0 - r2) / float(n - J - 2)) / 1e6
    p = assoc.erfc(math.sqrt(chisq / 2.0))
    return n, freq, (beta, se, chisq, p), False


def output_text(stats, loci_cols, names, empty="!"):
    """the --assoc file of stats[r][k] = stat(...) -> (bytes, tested, collinear)"""
    out = [assoc.HEADER]
    tested = collinear = 0
    for r, row in enumerate(stats):
        for k, (n, freq, st, col) in enumerate(row):
            f = list(loci_cols[r]) + [names[k].decode(), str(n), empty if freq is None else assoc.g3(freq)]
            f += [empty] * 4 if st is None else [assoc.g3(x) for x in st]
            tested += st is not None
            collinear += col
            out.append("\t".join(f))
    return ("\n".join(out) + "\n").encode(), tested, collinear


def report_text(k, n_named, rows, tested, j, incomplete, collinear):
    return assoc.report_text(k, n_named, rows, tested) + ("covariates\t%d\nincomplete\t%d\ncollinear\t%d\n" % (j, incomplete, collinear)).encode()


class Expected:
    pass


def expected_m(H, O, M, loci_cols, sample_names, pheno_text, covar_text, empty="!"):
    """everything a run with --covar gives, of class matrices"""
    e = Expected()
    e.names, Y, P, e.n_named = assoc.parse_file(pheno_text, sample_names)
    e.cnames, e.C, e.complete, e.c_named = parse_file(covar_text, sample_names)
    e.Y, e.P = mask(Y, P, e.complete)
    e.lay, e.group_of, e.first = layout_of(e.C, e.Y, e.P)
    e.recs = assoc.records(H, O, M, e.Y, e.P)
    e.tots = assoc.totals(e.Y, e.P)
    e.words = cov_words(H, O, M, e.C, e.Y, e.P, e.lay, e.group_of, e.first)
    e.tot_row = totals_row(e.C, e.Y, e.P, e.lay, e.group_of, e.first)
    J = len(e.C)
    e.stats = [[stat(gram(H[r], O[r], M[r], e.C, e.Y[k], e.P[k]), J) for k in range(len(e.Y))] for r in range(H.shape[0])]
    e.out, e.tested, e.collinear = output_text(e.stats, loci_cols, e.names, empty)
    e.incomplete = len(e.complete) - sum(e.complete)
    e.report = report_text(len(e.names), e.n_named, len(e.recs), e.tested, J, e.incomplete, e.collinear)
    return e


def expected(oracle_run, vcf, pheno_text, covar_text, cfg=None):
    """the same of a VCF through the oracle; .body and .log are the oracle's TSV and log"""
    cfg = cfg or {}
    rc, body, log, _ = oracle_run(vcf, cfg)
    assert rc == 0
    sn = pt.sample_names(vcf)
    H, O, M = pt.matrices(body, sn, cfg)
    e = expected_m(H, O, M, assoc.loci_columns(body), sn, pheno_text, covar_text, cfg.get("emptyField", "!"))
    e.body, e.log = body, log
    return e


# ---- inputs

def covar_rows(sample_names, j, seed, top=3 * assoc.ONE, na=0.03, absent=0.03, extra=(b"NOBODY",)):
    """a file's rows over the samples: J covariates of mixed sign up to `top` in size, some NA, some samples not named"""
    rng = random.Random(seed)
    sample_names = [x.encode() if isinstance(x, str) else x for x in sample_names]
    rows = []
    for nm in list(sample_names) + list(extra):
        if nm in sample_names and rng.random() < absent:
            continue
        rows.append((nm, [None if rng.random() < na else rng.randint(-top, top) for _ in range(j)]))
    rng.shuffle(rows)
    return rows


def covar_for(vcf, j, seed, names=None, **kw):
    return file_text(covar_rows(pt.sample_names(vcf), j, seed, **kw), names)
