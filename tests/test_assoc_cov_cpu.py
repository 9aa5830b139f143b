"""--covar without a device: the covariate file's rules, the table's groups, totals and operand B, the Gram matrix and the
statistic agree with the definition written in Python (assoc_cov.py); the structs match the header; the CLI refuses what it
must; the model means what it says (numpy.linalg.lstsq); and bvcf_assoc_cov_q.h -- the arithmetic the kernels, the table
builder and the writer share -- runs clean in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import assoc
import assoc_cov as ac
import variantlist as vl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bystro-vcf_amd", "csrc")
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


NAMES = [b"s0", b"s1", b"s2", b"s3", b"dup", b"dup"]


def both(bv, text, names=NAMES):
    """(model, library): ("ok", names, C, complete, named) / ("bad", line)"""
    out = []
    try:
        n, c, comp, named = ac.parse_file(text, names)
        out.append(("ok", n, c, comp, named))
    except ac.CovarFileError as e:
        out.append(("bad", e.line))
    try:
        t = bv.CovarTable(text=text, sample_names=names)
        out.append(("ok", t.names, t.c.tolist(), t.complete.tolist(), t.n_named))
        assert t.n_columns == 0 and t.row_words == 0 and t.n_incomplete == len(names) - int(t.complete.sum())
        t.close()
    except bv.BvcfError as e:
        msg = str(e).split(": ", 1)[1]
        out.append(("bad", int(msg.split(":")[0].split()[1]) if msg.startswith("line ") else 0))
    return tuple(out)


# ---- the file

ACCEPTED = [
    b"s0\t1\t2\ns1\t-0.5\tNA\n",                                  # no header: COV1, COV2; an NA makes s1 incomplete
    b"#sample\tage\tsex\r\ns1\t40\t1\r\n\r\ns0\t1e-6\t-1E+6\r\n",   # a header, CRLF, an empty line
    b"#FID\tIID\tPC1\tPC2\nf\ts2\t0.0123457\t-1.23457E-05\nf\ts3\t1\t0\nf\tghost\t1\t1\n",  # --pca's .eigenvec as it stands
    b"#sample\tc\n",                                              # a header alone: everybody incomplete
    b"nobody\t1\ns3\t2",                                          # a name no sample has, no newline at the end
    b"#sample\t" + b"\t".join(b"c%d" % i for i in range(16)) + b"\ns0" + b"\t1" * 16 + b"\n",  # J = 16
    b"#FID\tx\ns0\t5\n",                                          # "#FID" without "IID" is no such header: refused below
]
REFUSED = [
    (b"", 0), (b"\n\r\n\n", 0),                                   # no non-empty line
    (b"s0\t1\n#sample\tc\n", 2),                                  # a '#' line behind the first
    (b"#sample\tc\ns0\t1\t2\n", 2), (b"s0\t1\t2\ns1\t1\n", 2),     # a wrong field count
    (b"#sample\tc\n\t1\n", 2), (b"#FID\tIID\tc\nf\t\t1\n", 2),     # an empty name
    (b"#sample\tc\ns0\t1\n\ns0\t2\n", 4),                          # a sample on two lines
    (b"#sample\tc\ndup\t1\n", 2),                                 # a name that matches two columns
    (b"#sample\tc\ns0\tx\n", 2), (b"s0\t1e7\n", 1), (b"s0\tna\n", 1), (b"ghost\t1,5\n", 1),  # a bad value, also on an ignored line
    (b"#sample\n", 1), (b"s0\n", 1), (b"#FID\tIID\n", 1),          # J = 0
    (b"s0" + b"\t1" * 17 + b"\n", 1),                             # J = 17
    (b"#sample\tc\tc\ns0\t1\t2\n", 1), (b"#sample\t\ns0\t1\n", 1), (b"#name\tc\ns0\t1\n", 1),  # header names
    (b"#FID\tx\ns0\t5\n", 1),
]


def test_file_rules(bv):
    for text in ACCEPTED[:-1]:
        m, l = both(bv, text)
        assert m[0] == "ok" and m == l, (text, m, l)
    m = ac.parse_file(ACCEPTED[0], NAMES)
    assert m[0] == [b"COV1", b"COV2"] and m[1][0][:2] == [10 ** 6, 0] and m[2][:2] == [1, 0] and m[3] == 2
    m = ac.parse_file(ACCEPTED[2], NAMES)
    assert m[0] == [b"PC1", b"PC2"] and m[1][0][2] == 12346 and m[1][1][2] == -12 and m[2] == [0, 0, 1, 1, 0, 0] and m[3] == 2
    assert ac.parse_file(ACCEPTED[3], NAMES)[2] == [0] * 6


@pytest.mark.parametrize("text,line", REFUSED)
def test_file_errors_name_their_line(bv, text, line):
    m, l = both(bv, text)
    assert m == ("bad", line) and l == ("bad", line), (text, m, l)


# ---- the table

def random_case(seed, S, J, K, top=3 * 10 ** 6, ytop=10 ** 7, patterns=None, na=0.05):
    """(C [J][S], complete, Y, P): masked data over S samples; patterns[k]: which presence pattern phenotype k follows"""
    rng = random.Random(seed)
    complete = [0 if rng.random() < na else 1 for _ in range(S)]
    Cv = [[rng.randint(-top, top) if complete[i] else 0 for i in range(S)] for _ in range(J)]
    patterns = patterns or list(range(K))
    pats = {p: [1 if rng.random() < 0.9 else 0 for _ in range(S)] for p in set(patterns)}
    P = [list(pats[patterns[k]]) for k in range(K)]
    Y = [[rng.randint(-ytop, ytop) for _ in range(S)] for _ in range(K)]
    Y, P = ac.mask(Y, P, complete)
    return Cv, complete, Y, P


def tables(bv, Cv, complete, Y, P):
    ph = bv.PhenoTable(Y, P)
    ct = bv.CovarTable(Cv, complete, pheno=ph)
    return ph, ct


def test_mask_groups_totals_and_unmasked_tables(bv):
    Cv, complete, Y, P = random_case(1, 70, 3, 4, patterns=[0, 1, 0, 1])
    raw = bv.PhenoTable(Y, [[1] * 70] * 4)
    ph = raw.masked(complete)
    assert ph.present.tolist() == [complete] * 4 and ph.totals == assoc.totals(*ac.mask(Y, [[1] * 70] * 4, complete))
    with pytest.raises(bv.BvcfError) as ei:  # a phenotype on an incomplete sample: not the masked table
        bv.CovarTable(Cv, complete, pheno=raw)
    assert ei.value.rc == bv.E_ARG
    ph2, ct = tables(bv, Cv, complete, Y, P)
    lay, group_of, first = ac.layout_of(Cv, Y, P)
    assert (ct.n_groups, ct.group_of, ct.group_first) == (2, [0, 1, 0, 1], [0, 1]) == (lay.G, group_of, first)
    assert (ct.lc, ct.lcc, ct.lcy, ct.row_words, ct.n_blocks) == (lay.lc, lay.lcc, lay.lcy, lay.w, lay.n_blocks)
    assert ct.totals.tolist() == ac.totals_row(Cv, Y, P, lay, group_of, first)
    assert ct.n_incomplete == 70 - sum(complete)
    for t in (raw, ph, ph2, ct):
        t.close()


# J, K, the largest |C|, the largest |Y| -> (lc, lcc, lcy): one limb; 6 / 11 / 11; seven limbs -- two values and padding per block
LIMB_CASES = [(1, 1, 127, 1, (1, 2, 1)), (16, 1, 10 ** 12, 10 ** 12, (6, 11, 11)), (2, 2, 10 ** 8, 10 ** 8, (4, 7, 7)),
              (2, 16, 1000, 1000, (2, 3, 3))]


@pytest.mark.parametrize("J,K,top,ytop,limbs", LIMB_CASES)
def test_operand_b(bv, J, K, top, ytop, limbs):
    """every value whole within a block of 16 columns, zero where P = 0, past S and in the padding, and the limbs sum to the
    value"""
    S = 70
    Cv, complete, Y, P = random_case(10 + J, S, J, K, top=top, ytop=ytop, patterns=[k % 3 for k in range(K)])
    Cv[0][complete.index(1)] = top
    i0 = next(i for i in range(S) if P[0][i])
    Cv[0][i0], Y[0][i0] = top, ytop
    ph, ct = tables(bv, Cv, complete, Y, P)
    lay, group_of, first = ac.layout_of(Cv, Y, P)
    assert (ct.lc, ct.lcc, ct.lcy) == limbs == (lay.lc, lay.lcc, lay.lcy)
    b = ct.b.astype(object)
    assert b.shape == (16 * lay.n_blocks, 128) and not b[:, S:].any()
    used = np.zeros(b.shape[0], dtype=bool)

    def check(col, n, want):
        assert col // 16 == (col + n - 1) // 16, "a value straddles a block"
        assert not used[col:col + n].any()
        used[col:col + n] = True
        got = [sum(int(b[col + a][i]) << (8 * a) for a in range(n)) for i in range(S)]
        assert got == want

    for g, f in enumerate(first):
        for j in range(J):
            check(lay.col_c(g, j), lay.lc, [c if p else 0 for c, p in zip(Cv[j], P[f])])
            for i in range(j + 1):
                check(lay.col_cc(g, i, j), lay.lcc, [x * y if p else 0 for x, y, p in zip(Cv[i], Cv[j], P[f])])
    for k in range(K):
        for j in range(J):
            check(lay.col_cy(k, j), lay.lcy, [c * y if p else 0 for c, y, p in zip(Cv[j], Y[k], P[k])])
    assert not b[~used].any(), "the padding columns are zero"
    ph.close()
    ct.close()


# ---- the Gram matrix and the statistic

def random_classes(rng, n_rows, S, miss=0.2):
    cls = np.array([[rng.choices([0, 1, 2, 3], [0.4, 0.25, 0.15, miss])[0] for _ in range(S)] for _ in range(n_rows)])
    return (cls == 1).astype(np.uint8), (cls == 2).astype(np.uint8), (cls == 3).astype(np.uint8)


def stat_cases():
    """[(tag, C, complete, Y, P, (H, O, M))]: random data of several shapes, and the edges"""
    out = []
    for seed, S, J, K, top, ytop in ((1, 40, 1, 1, 127, 10 ** 6), (2, 70, 3, 2, 3 * 10 ** 6, 10 ** 7), (3, 30, 5, 3, 10 ** 12, 10 ** 12),
                                     (4, 25, 16, 1, 10 ** 6, 10 ** 6), (5, 90, 2, 16, 10 ** 9, 10 ** 3)):
        rng = random.Random(seed)
        Cv, complete, Y, P = random_case(seed, S, J, K, top=top, ytop=ytop, patterns=[k % 2 for k in range(K)])
        out.append(("random%d" % seed, Cv, complete, Y, P, random_classes(rng, 12, S)))
    rng = random.Random(50)
    S = 40
    Cv, complete, Y, P = random_case(50, S, 2, 2, na=0)
    Cv[1] = [2 * x for x in Cv[0]]
    out.append(("c2 = 2 c1", Cv, complete, Y, P, random_classes(rng, 6, S)))
    Cv, complete, Y, P = random_case(51, S, 2, 1, na=0)
    Cv[0] = [7 * 10 ** 6] * S
    out.append(("constant covariate", Cv, complete, Y, P, random_classes(rng, 6, S)))
    Cv, complete, Y, P = random_case(52, S, 3, 1, na=0)
    H, O, M = random_classes(rng, 6, S)
    M[:, 5:] = 1  # five called samples: n < J + 3
    H[:, 5:] = O[:, 5:] = 0
    out.append(("n < J + 3", Cv, complete, Y, P, (H, O, M)))
    Cv, complete, Y, P = random_case(53, S, 2, 2, na=0)
    P[1] = [0] * S
    Y[1] = [0] * S
    out.append(("a phenotype nobody has", Cv, complete, Y, P, random_classes(rng, 4, S)))
    Cv, complete, Y, P = random_case(54, 1, 1, 1, na=0)
    out.append(("one sample", Cv, complete, [[5]], [[1]], (np.array([[1]], dtype=np.uint8), np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8))))
    Cv, complete, Y, P = random_case(55, S, 2, 1, na=0)
    H, O, M = random_classes(rng, 4, S, miss=0.0)
    H[0, :] = O[0, :] = 0                     # nobody carries: the genotype's pivot is zero
    Y[0] = [3 * Cv[0][i] - Cv[1][i] + 10 ** 6 if P[0][i] else 0 for i in range(S)]  # y in the covariates' span: rss0 is not usable
    out.append(("monomorphic row, y collinear", Cv, complete, Y, P, (H, O, M)))
    return out


def test_statistic_against_the_model(bv):
    """bvcf_assoc_cov_stat from the records against the model from the definition, bit for bit; the two ways to the Gram matrix
    agree"""
    seen = {"tested": 0, "collinear": 0, "untested": 0, "short": 0}
    for tag, Cv, complete, Y, P, (H, O, M) in stat_cases():
        ph, ct = tables(bv, Cv, complete, Y, P)
        lay, group_of, first = ac.layout_of(Cv, Y, P)
        recs = assoc.records(H, O, M, Y, P)
        tots = assoc.totals(Y, P)
        words = ac.cov_words(H, O, M, Cv, Y, P, lay, group_of, first)
        tot_row = ac.totals_row(Cv, Y, P, lay, group_of, first)
        J = len(Cv)
        for r in range(H.shape[0]):
            for k in range(len(Y)):
                G = ac.gram(H[r], O[r], M[r], Cv, Y[k], P[k])
                assert G == ac.gram_of_records(recs[r][k], tots[k], words[r], tot_row, lay, k, group_of[k]), (tag, r, k)
                n, freq, st, col = ac.stat(G, J)
                flags, out = bv.assoc_cov_stat(ct, k, recs[r][k], tots[k], words[r])
                assert flags == (freq is not None) + 2 * (st is not None) + 4 * col, (tag, r, k, flags)
                want = [float(n), freq or 0.0] + (list(st) if st else [0.0] * 4)
                assert [x.hex() for x in out] == [x.hex() for x in want], (tag, r, k)
                seen["tested" if st else "collinear" if col else "short" if n < J + 3 else "untested"] += 1
                if tag in ("c2 = 2 c1", "constant covariate") and n >= J + 3:
                    assert col and st is None, tag
                if tag in ("n < J + 3", "a phenotype nobody has", "one sample") and (tag != "a phenotype nobody has" or k == 1):
                    assert st is None and not col, tag
        ph.close()
        ct.close()
    assert seen["tested"] > 100 and seen["collinear"] > 8 and seen["short"] > 8 and seen["untested"] > 0, seen


def test_refusals_of_the_stat(bv):
    Cv, complete, Y, P = random_case(2, 20, 2, 1)
    ph, ct = tables(bv, Cv, complete, Y, P)
    un = bv.CovarTable(Cv, complete)
    rec, tot = (0, 0, 0, 0, 0, 0, 0), assoc.totals(Y, P)[0]
    assert bv.assoc_cov_stat(ct, 1, rec, tot, [0] * ct.row_words)[0] == -1  # k >= K
    un.t.row_words = ct.row_words
    assert bv.assoc_cov_stat(un, 0, rec, tot, [0] * ct.row_words)[0] == -1  # an unbound table
    un.t.row_words = 0
    for t in (ph, ct, un):
        t.close()


def test_model_against_lstsq():
    """what the numbers mean: beta and se of the model against an ordinary least-squares fit of y on (1, C, g) over the called
    samples, on well-conditioned random data.  The bound is eight times the largest relative deviation measured with this
    very test on the CPU (assoc_cov.LSTSQ_MEASURED), never taken from the device"""
    worst = 0.0
    for seed in ac.LSTSQ_SEEDS:
        rng = random.Random(seed)
        S, J = 200, 1 + seed % 5
        Cv = [[rng.randint(-3 * 10 ** 6, 3 * 10 ** 6) for _ in range(S)] for _ in range(J)]
        H, O, M = random_classes(rng, 4, S, miss=0.1)
        g_all = H.astype(int) + 2 * O.astype(int)
        for r in range(4):
            y = [int(10 ** 6 * (0.3 * g_all[r][i] + sum(0.2 * (q + 1) * Cv[q][i] / 10 ** 6 for q in range(J)) + rng.gauss(0, 1))) for i in range(S)]
            n, freq, st, col = ac.stat(ac.gram(H[r], O[r], M[r], Cv, y, [1] * S), J)
            idx = [i for i in range(S) if not M[r][i]]
            X = np.array([[1.0] + [Cv[q][i] / 1e6 for q in range(J)] + [float(g_all[r][i])] for i in idx])
            yy = np.array([y[i] / 1e6 for i in idx])
            coef, res, rank, _ = np.linalg.lstsq(X, yy, rcond=None)
            assert rank == J + 2 and st is not None
            resid = yy - X @ coef
            # the score test's se uses the residual variance of the model WITH g over n - J - 2 degrees of freedom
            se = np.sqrt(resid @ resid / (len(idx) - J - 2) * np.linalg.inv(X.T @ X)[J + 1, J + 1])
            worst = max(worst, abs(st[0] - coef[J + 1]) / abs(coef[J + 1]), abs(st[1] - se) / se)
    print("largest relative deviation of beta / se from lstsq: %.3e (bound %.3e)" % (worst, ac.LSTSQ_BOUND))
    assert worst <= ac.LSTSQ_BOUND


# ---- the header, the structs, the config

def test_header_and_exports(bv):
    hdr = open(os.path.join(ROOT, "include", "bvcf.h")).read()
    for name in ("bvcf_covar_table_parse", "bvcf_covar_table_build", "bvcf_covar_table_free", "bvcf_pheno_table_mask", "bvcf_set_covar_table",
                 "bvcf_assoc_cov", "bvcf_assoc_cov_stat", "bvcf_config_covar_defaults"):
        assert name + "(" in hdr and name in bv.EXPORTS
        getattr(bv.lib, name)
    assert "bvcf_bench_assoc_cov_kernels" in bv.BENCH_EXPORTS
    assert "#define BVCF_CONFIG_MORE_COVAR 11" in hdr and bv.CONFIG_MORE_COVAR == 11
    assert "#define BVCF_ABI_VERSION %d" % bv.ABI_VERSION in hdr or bv.ABI_VERSION == 9  # (additive: no version bump)


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(bvcf_covar_table),sizeof(bvcf_assoc_cov_info),sizeof(bvcf_config_covar),offsetof(bvcf_config_covar,covar_path),"
                   "offsetof(bvcf_covar_table,totals),sizeof(bvcf_config_pca),sizeof(bvcf_assoc_rec));return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [C.sizeof(bv.CovarTableStruct), C.sizeof(bv.AssocCovInfo), C.sizeof(bv.ConfigCovar), bv.ConfigCovar.covar_path.offset,
                   bv.CovarTableStruct.totals.offset, C.sizeof(bv.ConfigPca), 56]


def test_config_markers(bv):
    c = bv.make_config({"pheno": "/p", "assoc": "/a", "pca": "/x"})
    assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_PCA]  # (the flag off: what the eleventh marker wrote)
    c = bv.make_config({"pheno": "/p", "assoc": "/a", "covar": "/c"})
    assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_COVAR]
    v = C.cast(C.byref(c), C.POINTER(bv.ConfigCovar)).contents
    assert (v.covar_path, v.pca.assoc.pheno_path, v.pca.pca_prefix) == (b"/c", b"/p", None)
    d = bv.ConfigCovar()
    bv.lib.bvcf_config_covar_defaults(C.byref(d))
    base = d.pca.assoc.score.grm.regions.variants.ld.trios.more.base
    assert list(base.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_COVAR] and d.covar_path is None and d.pca.pca_count == bv.PCA_DEFAULT_COMPONENTS
    p = bv.ConfigPca()
    bv.lib.bvcf_config_pca_defaults(C.byref(p))
    assert list(p.assoc.score.grm.regions.variants.ld.trios.more.base.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_PCA]


# ---- the CLI, as far as it gets without a device

def cli(args, stdin_bytes=b""):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=60)


def test_cli_flag_without_a_value_or_its_partners():
    p = cli(["--covar"])
    assert p.returncode == 2 and p.stdout == b"" and p.stderr == b"flag needs an argument: -covar\n"
    p = cli(["--covar="])
    assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1
    for args in (["--covar", "c"], ["--covar", "c", "--pheno", "p"], ["--covar", "c", "--assoc", "a"]):
        p = cli(args, vl.rows_vcf(5))
        assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1, args


# ---- the shared header under sanitizers

def fmt(x):
    return float(x).hex()


def test_arithmetic_header_alone_under_sanitizers(tmp_path):
    """bvcf_assoc_cov_q.h in a program of its own: the layout, the Gram matrix from the records and the statistic bit for bit"""
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present: sanitized programs run on the build machine")
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "assoc_cov_check")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "assoc_cov_check.cpp"),
                           "-o", exe], timeout=120)
    m64 = (1 << 64) - 1
    lines, want = [], []
    for tag, Cv, complete, Y, P, (H, O, M) in stat_cases():
        lay, group_of, first = ac.layout_of(Cv, Y, P)
        recs = assoc.records(H, O, M, Y, P)
        tots = assoc.totals(Y, P)
        words = ac.cov_words(H, O, M, Cv, Y, P, lay, group_of, first)
        tot_row = ac.totals_row(Cv, Y, P, lay, group_of, first)
        J, K = len(Cv), len(Y)
        for r in range(H.shape[0]):
            for k in range(K):
                rec, tot = recs[r][k], tots[k]
                f = [J, K, lay.G, lay.lc, lay.lcc, lay.lcy, k, group_of[k]] + [x & m64 for x in rec[:6]] + [rec[6] & m64, rec[6] >> 64]
                f += [tot[0], tot[1] & m64, tot[2] & m64, tot[2] >> 64] + words[r] + tot_row
                lines.append(" ".join(str(x) for x in f))
                n_slices_c = -(-lay.bc // 5)
                want.append(" ".join(str(x) for x in ["layout", lay.w, lay.n_blocks, n_slices_c, n_slices_c + -(-(lay.bcc + lay.bcy) // 16),
                                                      lay.col_c(0, 0), lay.col_c(lay.G - 1, J - 1), lay.word_c(0, 0, 0), lay.word_c(lay.G - 1, 2, J - 1),
                                                      lay.col_cc(0, 0, 0), lay.col_cc(lay.G - 1, J - 1, J - 1), lay.word_cc(0, 0, 0),
                                                      lay.word_cc(lay.G - 1, J - 1, J - 1), lay.col_cy(0, 0), lay.col_cy(K - 1, J - 1),
                                                      lay.word_cy(0, 0), lay.word_cy(K - 1, J - 1)]))
                G = ac.gram_of_records(rec, tot, words[r], tot_row, lay, k, group_of[k])
                n, freq, st, col = ac.stat(G, J)
                six = [float(n), freq or 0.0] + (list(st) if st else [0.0] * 4)
                want.append(" ".join([str(x) for row in G for x in row] + [str((freq is not None) + 2 * (st is not None) + 4 * col)] +
                                     [fmt(x) for x in six]))
    (tmp_path / "c.txt").write_text("".join(x + "\n" for x in lines))
    p = subprocess.run([exe, str(tmp_path / "c.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.endswith("assoc_cov_q ok\n"), out[-2000:]
    assert "ERROR" not in out and "runtime error" not in out, out[-2000:]

    def canon(line):  # (C's %a and float.hex() spell the same double differently)
        return " ".join(fmt(float.fromhex(x)) if "x" in x or x in ("inf", "-inf") else x for x in line.split(" "))
    got = out.split("\n")[:-2]
    assert len(got) == len(want) > 200
    assert [canon(x) for x in got] == [canon(x) for x in want]
