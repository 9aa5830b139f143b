"""--assocModel logistic: the null fit, the fixed-point vectors, the expected records and both output files of the logistic
score test, written from the rules of include/bvcf.h alone and built from the oracle's TSV of the same bytes.

The fit runs operation for operation in Python floats with exp and erfc from the same libm through ctypes; round() gives M
(ties to even); a row's heterozygotes / homozygotes / missingGenos lists give the classes; every sum is a Python integer;
float(int) is the correctly rounded double.  The matrix G is summed straight from its definition over the sample set (gram);
gram_of_records puts it together from the records and the totals as the library does, and the tests hold the two against
each other.  Test infrastructure only."""
import ctypes
import ctypes.util
import math
import random

import numpy as np

import assoc
import assoc_cov as ac
import pairtable as pt

ONE = 1 << 24
MAX_ROUNDS = 25
TINY = 2.0 ** -30

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.exp.restype = ctypes.c_double
_libm.exp.argtypes = [ctypes.c_double]

# The model's chisq (fixed point, 2^-24) against the same formula in unquantised numpy doubles
# (test_assoc_logit_cpu.py::test_meaning_against_unquantised_doubles, seeds MEANING_SEEDS, S in MEANING_S, J in MEANING_J): the
# largest relative deviation measured there, on the CPU, and the bound the test asserts -- eight times that value, the rule of
# tests/pca.py.  Never taken from the device.
MEANING_SEEDS = [9300, 9301, 9302]
MEANING_S = [50, 200, 2000]
MEANING_J = [0, 1, 3, 10]
MEANING_MEASURED = 4.334e-06
MEANING_BOUND = 8 * MEANING_MEASURED
# With J = 0 on rows without missing calls the model's chisq against the linear scan's (Cochran-Armitage, assoc.stat), measured
# and bounded the same way (test_j0_equals_the_trend_test, seeds TREND_SEEDS)
TREND_SEEDS = [9400, 9401, 9402, 9403]
TREND_MEASURED = 3.422e-07
TREND_BOUND = 8 * TREND_MEASURED


def exp(x):
    return _libm.exp(x)


# ---- the null fit

def mu_of(beta, xi):
    eta = beta[0]
    for j in range(1, len(beta)):
        eta = eta + beta[j] * xi[j]
    return 1.0 / (1.0 + exp(-eta))


def fit(x, y, J):
    """x [n][J+1] floats (x_i0 = 1.0), y [n] 1.0 / 0.0 -> (fitted, beta, rounds): include/bvcf.h's rounds, operation for operation"""
    m = J + 1
    beta = [0.0] * m
    for rounds in range(1, MAX_ROUNDS + 1):
        H = [[0.0] * m for _ in range(m + 1)]
        for xi, yi in zip(x, y):
            mu = mu_of(beta, xi)
            w = mu * (1.0 - mu)
            r = yi - mu
            for a in range(m):
                wx = w * xi[a]
                for b in range(a + 1):
                    H[a][b] = H[a][b] + wx * xi[b]
                H[m][a] = H[m][a] + xi[a] * r
        u = [[0.0] * m for _ in range(m + 1)]
        L = [[0.0] * m for _ in range(m + 1)]
        d = [0.0] * m
        for a in range(m + 1):
            for b in range(min(a, m)):
                s = H[a][b]
                for t in range(b):
                    s = s - u[a][t] * L[b][t]
                u[a][b] = s
                L[a][b] = s / d[b]
            if a == m:
                break
            s = H[a][a]
            for t in range(a):
                s = s - u[a][t] * L[a][t]
            d[a] = s
            if not d[a] > H[a][a] * TINY:
                return False, beta, rounds
        delta = [0.0] * m
        for b in range(m - 1, -1, -1):
            s = L[m][b]
            for t in range(b + 1, m):
                s = s - L[t][b] * delta[t]
            delta[b] = s
        conv = True
        for a in range(m):
            beta[a] = beta[a] + delta[a]
            if not math.isfinite(beta[a]):
                return False, beta, rounds
            if not abs(delta[a]) <= 1e-10:
                conv = False
        if conv:
            return True, beta, rounds
    return False, beta, MAX_ROUNDS


def x_rows(Cv, p):
    """the samples of Omega in ascending index and their rows x"""
    omega = [i for i in range(len(p)) if p[i]]
    return omega, [[1.0] + [float(c[i]) / 1e6 for c in Cv] for i in omega]


class Null:
    """the K null models of masked data: fitted [K], beta [K], rounds [K], mu [K] {sample: float}, M / R / W [K][S] integers"""

    def __init__(self, Cv, Y, P):
        K, S = len(Y), len(P[0]) if P else 0
        J = len(Cv)
        self.fitted, self.beta, self.rounds, self.mu = [], [], [], []
        self.M = [[0] * S for _ in range(K)]
        self.R = [[0] * S for _ in range(K)]
        self.W = [[0] * S for _ in range(K)]
        for k in range(K):
            omega, x = x_rows(Cv, P[k])
            y = [1.0 if Y[k][i] else 0.0 for i in omega]
            ok, beta, rounds = fit(x, y, J)
            self.fitted.append(ok)
            self.beta.append(beta)
            self.rounds.append(rounds)
            self.mu.append({})
            if not ok:
                continue
            for i, xi, yi in zip(omega, x, y):
                mu = mu_of(beta, xi)
                self.mu[k][i] = mu
                m = round(mu * 16777216.0)  # (the product is exact; round() goes to the even neighbour on a tie)
                assert 0 <= m <= ONE
                self.M[k][i] = m
                self.R[k][i] = (ONE if yi else 0) - m
                self.W[k][i] = (m * (ONE - m)) >> 24
        self.n_unfitted = sum(1 for f in self.fitted if not f)


def check_binary(names, Y, P, sample_names):
    """(phenotype name, sample name) of the first present value that is neither 0 nor 1, or None"""
    for k, (y, p) in enumerate(zip(Y, P)):
        for i, (v, q) in enumerate(zip(y, p)):
            if q and v not in (0, assoc.ONE):
                return names[k], sample_names[i]
    return None


# ---- the layout

class Layout:
    """where a logistic record's words and operand B's columns are (include/bvcf.h)"""

    def __init__(self, J, K, lwc, lr, lrc, lwcc):
        self.J, self.K, self.lwc, self.lr, self.lrc, self.lwcc = J, K, lwc, lr, lrc, lwcc
        self.j1 = J + 1
        self.np2 = J * (J + 1) // 2
        self.pv = 4 * self.j1 + 2 + self.np2
        self.w = 2 * K * self.pv
        self.vwc, self.vr, self.vrc, self.vwcc = 16 // lwc, 16 // lr, 16 // lrc, 16 // lwcc
        self.nwc, self.nr, self.nrc, self.nwcc = K * self.j1, K, K * self.j1, K * self.np2
        self.bwc, self.br, self.brc, self.bwcc = (-(-n // v) for n, v in ((self.nwc, self.vwc), (self.nr, self.vr), (self.nrc, self.vrc),
                                                                         (self.nwcc, self.vwcc)))
        self.n_blocks = self.bwc + self.br + self.brc + self.bwcc

    def word_wc(self, k, cls, a):
        return 2 * (k * self.pv + cls * self.j1 + a)

    def word_r(self, k, cls):
        return 2 * (k * self.pv + 3 * self.j1 + cls)

    def word_rc(self, k, a):
        return 2 * (k * self.pv + 3 * self.j1 + 2 + a)

    def word_wcc(self, k, a, b):
        """1 <= a <= b <= J"""
        return 2 * (k * self.pv + 4 * self.j1 + 2 + (b - 1) * b // 2 + (a - 1))

    @staticmethod
    def _col(first, per, limbs, v):
        return 16 * (first + v // per) + (v % per) * limbs

    def col_wc(self, k, a):
        return self._col(0, self.vwc, self.lwc, k * self.j1 + a)

    def col_r(self, k):
        return self._col(self.bwc, self.vr, self.lr, k)

    def col_rc(self, k, a):
        return self._col(self.bwc + self.br, self.vrc, self.lrc, k * self.j1 + a)

    def col_wcc(self, k, a, b):
        return self._col(self.bwc + self.br + self.brc, self.vwcc, self.lwcc, k * self.np2 + (b - 1) * b // 2 + (a - 1))


def c_of(Cv, a, i):
    return Cv[a - 1][i] if a else 1


def layout_of(Cv, nul, P):
    """the smallest limb counts that hold the table's values, over the samples of each phenotype"""
    J, K = len(Cv), len(P)
    lwc = lr = lrc = lwcc = 1
    for k in range(K):
        for i, p in enumerate(P[k]):
            if not p:
                continue
            w, r = nul.W[k][i], nul.R[k][i]
            lr = max(lr, assoc.n_limbs(r))
            for a in range(J + 1):
                lwc = max(lwc, assoc.n_limbs(w * c_of(Cv, a, i)))
                lrc = max(lrc, assoc.n_limbs(r * c_of(Cv, a, i)))
                for b in range(max(a, 1), J + 1 if a else 0):
                    lwcc = max(lwcc, assoc.n_limbs(w * c_of(Cv, a, i) * c_of(Cv, b, i)))
    return Layout(J, K, lwc, lr, lrc, lwcc)


def operand_b(Cv, nul, P, lay):
    """int8 [16 n_blocks][s64]"""
    S = len(P[0]) if P else 0
    s64 = (S + 63) & ~63
    B = np.zeros((16 * lay.n_blocks, s64), dtype=np.int8)

    def put(col, limbs, i, v):
        for q, d in enumerate(assoc.limbs(v, limbs)):
            B[col + q][i] = d

    for k in range(lay.K):
        for i in range(S):
            if not P[k][i]:
                continue
            w, r = nul.W[k][i], nul.R[k][i]
            put(lay.col_r(k), lay.lr, i, r)
            for a in range(lay.J + 1):
                put(lay.col_wc(k, a), lay.lwc, i, w * c_of(Cv, a, i))
                put(lay.col_rc(k, a), lay.lrc, i, r * c_of(Cv, a, i))
                for b in range(max(a, 1), lay.J + 1 if a else 0):
                    put(lay.col_wcc(k, a, b), lay.lwcc, i, w * c_of(Cv, a, i) * c_of(Cv, b, i))
    return B


# ---- the records

def _sums(cls, vec):
    """[rows] exact sums of vec (Python integers of any size) over the samples of a class matrix [rows][S]"""
    n_rows, S = cls.shape
    tot = [0] * n_rows
    if not S:
        return tot
    top = max(abs(v) for v in vec)
    for j in range(top.bit_length() // 21 + 1):  # 21-bit pieces: every int64 product is exact
        piece = np.array([(1 if v >= 0 else -1) * ((abs(v) >> (21 * j)) & ((1 << 21) - 1)) for v in vec], dtype=np.int64)
        if piece.any():
            tot = [t + (x << (21 * j)) for t, x in zip(tot, (cls @ piece).tolist())]
    return tot


def _u64(v):
    return v & ((1 << 64) - 1)


def logit_words(H, O, M, Cv, nul, P, lay):
    """[rows][W] the logistic records as unsigned 64-bit words"""
    n_rows = H.shape[0]
    out = [[0] * lay.w for _ in range(n_rows)]
    cls = [x.astype(np.int64) for x in (H, O, M)]
    S = H.shape[1]

    def put(at, vals):
        for r, v in enumerate(vals):
            out[r][at] = _u64(v)
            out[r][at + 1] = _u64(v >> 64)

    for k in range(lay.K):
        inn = [i for i in range(S)]
        W = [nul.W[k][i] if P[k][i] else 0 for i in inn]
        R = [nul.R[k][i] if P[k][i] else 0 for i in inn]
        for a in range(lay.J + 1):
            wc = [w * c_of(Cv, a, i) for i, w in enumerate(W)]
            for c in range(3):
                put(lay.word_wc(k, c, a), _sums(cls[c], wc))
            put(lay.word_rc(k, a), _sums(cls[2], [r * c_of(Cv, a, i) for i, r in enumerate(R)]))
            for b in range(max(a, 1), lay.J + 1 if a else 0):
                put(lay.word_wcc(k, a, b), _sums(cls[2], [x * c_of(Cv, b, i) for i, x in enumerate(wc)]))
        for c in range(2):
            put(lay.word_r(k, c), _sums(cls[c], R))
    return out


def totals_row(Cv, nul, P, lay):
    """[W] the totals row: the sums over all of Omega in the missing-class places, zero in the het / hom places"""
    S = len(P[0]) if P else 0
    ones = np.ones((1, S), dtype=np.int64)
    zero = np.zeros((1, S), dtype=np.int64)
    return logit_words(zero, zero, ones, Cv, nul, P, lay)[0]


# ---- the statistic

def gram(h, o, m, Cv, nul, k, p):
    """G (lower triangle, rows 0 .. J + 2, Python integers) of one row (class vectors h, o, m) and phenotype k, straight from
    the definition: v_0 = 1, v_1 .. v_J = C_j, v_{J+1} = g over {P = 1 and called}; G[a][b] = sum W v_a v_b, the last row
    sum R v_b"""
    J = len(Cv)
    idx = [i for i in range(len(p)) if p[i] and not m[i]]
    V = [[1] * len(idx)] + [[c[i] for i in idx] for c in Cv] + [[int(h[i]) + 2 * int(o[i]) for i in idx]]
    W = [nul.W[k][i] for i in idx]
    R = [nul.R[k][i] for i in idx]
    G = [[sum(w * x * y for w, x, y in zip(W, V[a], V[b])) for b in range(a + 1)] for a in range(J + 2)]
    G.append([sum(r * x for r, x in zip(R, V[b])) for b in range(J + 2)] + [0])
    return G


def _i128(words, at):
    v = (words[at + 1] << 64) | words[at]
    return v - (1 << 128) if v >> 127 else v


def gram_of_records(row, tot_row, lay, k):
    """the same matrix from the row's logistic words and the totals row: a total minus what was summed over the missing
    samples, or a sum over het / hom"""
    J = lay.J
    G = [[0] * (a + 1) for a in range(J + 3)]
    for a in range(J + 1):
        G[a][0] = _i128(tot_row, lay.word_wc(k, 2, a)) - _i128(row, lay.word_wc(k, 2, a))
        G[J + 1][a] = _i128(row, lay.word_wc(k, 0, a)) + 2 * _i128(row, lay.word_wc(k, 1, a))
        G[J + 2][a] = _i128(tot_row, lay.word_rc(k, a)) - _i128(row, lay.word_rc(k, a))
        for b in range(1, a + 1):
            G[a][b] = _i128(tot_row, lay.word_wcc(k, b, a)) - _i128(row, lay.word_wcc(k, b, a))
    G[J + 1][J + 1] = _i128(row, lay.word_wc(k, 0, 0)) + 4 * _i128(row, lay.word_wc(k, 1, 0))
    G[J + 2][J + 1] = _i128(row, lay.word_r(k, 0)) + 2 * _i128(row, lay.word_r(k, 1))
    return G


def stat(G, J, n, sg, fitted):
    """(n, altFreq or None, (beta, se, chisq, p) or None, collinear): the sequence of include/bvcf.h, operation for operation"""
    freq = float(sg) / float(2 * n) if n > 0 else None
    if not fitted or n < J + 3:
        return n, freq, None, False
    m = J + 3
    D = [[float(G[a][b]) for b in range(a + 1)] for a in range(m)]
    u = [[0.0] * m for _ in range(m)]
    L = [[0.0] * m for _ in range(m)]
    d = [0.0] * m
    for a in range(m):
        for b in range(a):
            s = D[a][b]
            for t in range(b):
                s = s - u[a][t] * L[b][t]
            u[a][b] = s
            L[a][b] = s / d[b]
        if a == J + 2:
            break
        s = D[a][a]
        for t in range(a):
            s = s - u[a][t] * L[a][t]
        d[a] = s
        if not d[a] > D[a][a] * TINY:
            return n, freq, None, a <= J
    V, ug = d[J + 1], u[J + 2][J + 1]
    beta = ug / V
    chisq = beta * (ug / 16777216.0)
    se = math.sqrt(16777216.0 / V)
    p = assoc.erfc(math.sqrt(chisq / 2.0))
    return n, freq, (beta, se, chisq, p), False


def chisq_unquantised(h, o, m, Cv, y, p, beta):
    """the score statistic of the same null model in numpy doubles, no fixed point: U^2 / V with U = g . (y - mu),
    V = g W g - g W X (X W X)^-1 X W g over {P = 1 and called}"""
    idx = [i for i in range(len(p)) if p[i] and not m[i]]
    X = np.array([[1.0] + [c[i] / 1e6 for c in Cv] for i in idx], dtype=np.float64)
    g = np.array([float(h[i]) + 2.0 * float(o[i]) for i in idx])
    yy = np.array([1.0 if y[i] else 0.0 for i in idx])
    mu = 1.0 / (1.0 + np.exp(-(X @ np.array(beta))))
    w = mu * (1.0 - mu)
    xwx = X.T @ (X * w[:, None])
    xwg = X.T @ (w * g)
    v = float(g @ (w * g) - xwg @ np.linalg.solve(xwx, xwg))
    # (the residual is orthogonal to X at the fit, so g's projection drops out of U up to the fit's 1e-10)
    uu = float((g - X @ np.linalg.solve(xwx, xwg)) @ (yy - mu))
    return uu * uu / v


def report_text(k, n_named, rows, tested, j, incomplete, collinear, unfitted):
    return ac.report_text(k, n_named, rows, tested, j, incomplete, collinear) + ("unfitted\t%d\n" % unfitted).encode()


class Expected:
    pass


def expected_m(H, O, M, loci_cols, sample_names, pheno_text, covar_text=None, empty="!"):
    """everything a run with --assocModel logistic gives, of class matrices"""
    e = Expected()
    e.names, Y, P, e.n_named = assoc.parse_file(pheno_text, sample_names)
    if covar_text is not None:
        e.cnames, e.C, e.complete, e.c_named = ac.parse_file(covar_text, sample_names)
        e.Y, e.P = ac.mask(Y, P, e.complete)
        e.incomplete = len(e.complete) - sum(e.complete)
    else:
        e.C, e.Y, e.P, e.incomplete = [], Y, P, 0
    J = len(e.C)
    e.bad = check_binary(e.names, e.Y, e.P, sample_names)
    if e.bad:
        return e
    e.nul = Null(e.C, e.Y, e.P)
    e.lay = layout_of(e.C, e.nul, e.P)
    e.recs = assoc.records(H, O, M, e.Y, e.P)
    e.tots = assoc.totals(e.Y, e.P)
    e.words = logit_words(H, O, M, e.C, e.nul, e.P, e.lay)
    e.tot_row = totals_row(e.C, e.nul, e.P, e.lay)
    e.stats = []
    for r in range(H.shape[0]):
        row = []
        for k in range(len(e.Y)):
            n_het, n_hom, n_mis = e.recs[r][k][:3]
            G = gram_of_records(e.words[r], e.tot_row, e.lay, k)
            row.append(stat(G, J, e.tots[k][0] - n_mis, n_het + 2 * n_hom, e.nul.fitted[k]))
        e.stats.append(row)
    e.out, e.tested, e.collinear = ac.output_text(e.stats, loci_cols, e.names, empty)
    e.report = report_text(len(e.names), e.n_named, len(e.recs), e.tested, J, e.incomplete, e.collinear, e.nul.n_unfitted)
    return e


def expected(oracle_run, vcf, pheno_text, covar_text=None, cfg=None):
    """the same of a VCF through the oracle; .body and .log are the oracle's TSV and log"""
    cfg = cfg or {}
    rc, body, log, _ = oracle_run(vcf, cfg)
    assert rc == 0
    sn = pt.sample_names(vcf)
    H, O, M = pt.matrices(body, sn, cfg)
    e = expected_m(H, O, M, assoc.loci_columns(body), sn, pheno_text, covar_text, cfg.get("emptyField", "!"))
    e.body, e.log, e.H, e.O, e.M = body, log, H, O, M
    return e


# ---- inputs

def binary_rows(sample_names, k, seed, na=0.08, absent=0.04, extra=(b"NOBODY",), unfitted_column=None):
    """a file's rows over the samples: K 0/1 columns of different prevalence, some NA, some samples not named; unfitted_column:
    a column that is 1 for everybody (its null model does not fit)"""
    rng = random.Random(seed)
    sample_names = [x.encode() if isinstance(x, str) else x for x in sample_names]
    rows = []
    for nm in list(sample_names) + list(extra):
        if nm in sample_names and rng.random() < absent:
            continue
        vs = []
        for c in range(k):
            if rng.random() < na:
                vs.append(None)
            elif c == unfitted_column:
                vs.append(assoc.ONE)
            else:
                vs.append(assoc.ONE if rng.random() < 0.25 + 0.5 * ((c * 7 + 3) % 10) / 10 else 0)
        rows.append((nm, vs))
    rng.shuffle(rows)
    return rows


def pheno_for(vcf, k, seed, names=None, **kw):
    return assoc.file_text(binary_rows(pt.sample_names(vcf), k, seed, **kw), names)
