"""--assocModel logistic without a device: the null fit, the fixed-point vectors, operand B and the statistic against the
model written from the rules (assoc_logit.py), bit for bit; what the numbers mean, against unquantised doubles and against
the linear scan's trend test; the refusal of a trait that is not 0 / 1; the struct and the flag; and the arithmetic header
in a stand-alone program under the address and undefined-behaviour sanitizers, bit-equal with the library."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import assoc
import assoc_cov as ac
import assoc_logit as al
import variantlist as vl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bystro-vcf_amd", "csrc")
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


# ---- the data

def random_case(seed, S, J, K, top=3 * 10 ** 6, na=0.05, effect=0.6):
    """(C [J][S], complete [S], masked Y and P [K][S]): 0/1 traits that lean on the first covariate"""
    rng = random.Random(seed)
    Cv = [[rng.randint(-top, top) for _ in range(S)] for _ in range(J)]
    complete = [0 if rng.random() < na else 1 for _ in range(S)]
    Cv = [[c if k else 0 for c, k in zip(row, complete)] for row in Cv]
    Y, P = [], []
    for k in range(K):
        P.append([1 if rng.random() > na else 0 for _ in range(S)])
        Y.append([assoc.ONE if rng.random() < 0.3 + 0.05 * k + (effect * 0.2 * Cv[0][i] / top if J else 0.0) else 0 for i in range(S)])
    if J:
        Y, P = ac.mask(Y, P, complete)
    else:
        Y = [[y if p else 0 for y, p in zip(a, b)] for a, b in zip(Y, P)]
    return Cv, complete, Y, P


def tables(bv, Cv, complete, Y, P):
    ph = bv.PhenoTable(Y, P)
    ct = bv.CovarTable(Cv, complete) if Cv else None
    return ph, ct, bv.LogitTable(ph, ct)


def close(*ts):
    for t in ts:
        if t is not None:
            t.close()


def random_classes(rng, n_rows, S, miss=0.2):
    cls = np.array([[3 if rng.random() < miss else rng.choice([0, 0, 0, 1, 1, 2]) for _ in range(S)] for _ in range(n_rows)]).reshape(n_rows, S)
    return cls == 1, cls == 2, cls == 3


# ---- 1. the fit

FIT_CASES = [(9200, 120, 0, 2), (9201, 150, 1, 2), (9202, 200, 3, 3), (9203, 400, 16, 1), (9204, 64, 3, 1), (9205, 1, 0, 1)]


@pytest.mark.parametrize("seed,S,J,K", FIT_CASES)
def test_fit_against_the_model(bv, seed, S, J, K):
    Cv, complete, Y, P = random_case(seed, S, J, K)
    ph, ct, lt = tables(bv, Cv, complete, Y, P)
    nul = al.Null(Cv, Y, P)
    assert lt.fitted == [int(x) for x in nul.fitted] and lt.rounds == nul.rounds and lt.n_unfitted == nul.n_unfitted
    for k in range(K):
        assert [x.hex() for x in lt.beta[k]] == [x.hex() for x in nul.beta[k]], k  # (bit for bit, unfitted ones too)
    assert lt.m.tolist() == nul.M and lt.r.tolist() == nul.R and lt.w.tolist() == nul.W
    if S > 1:
        assert all(nul.fitted) and all(2 <= r <= 10 for r in nul.rounds)
    close(ph, ct, lt)


def test_traits_and_covariates_that_do_not_fit(bv):
    """a separated trait (y = [c > 0]), an all-0 and an all-1 trait, nobody with the trait, and a covariate twice: unfitted,
    with M = R = W = 0 everywhere; a plain trait beside them fits"""
    rng = random.Random(9210)
    S = 90
    c = [rng.randint(-10 ** 6, 10 ** 6) or 1 for _ in range(S)]
    Y = [[assoc.ONE if x > 0 else 0 for x in c], [0] * S, [assoc.ONE] * S, [0] * S, [assoc.ONE if rng.random() < 0.4 else 0 for _ in range(S)]]
    P = [[1] * S, [1] * S, [1] * S, [0] * S, [1] * S]
    ph, ct, lt = tables(bv, [c], [1] * S, Y, P)
    nul = al.Null([c], Y, P)
    assert nul.fitted == [False, False, False, False, True] and lt.fitted == [0, 0, 0, 0, 1] and lt.n_unfitted == 4
    assert nul.rounds[:4] == [25, 25, 25, 1] and lt.rounds == nul.rounds
    assert lt.m.tolist() == nul.M and lt.r.tolist() == nul.R and lt.w.tolist() == nul.W
    assert not lt.m[:4].any() and not lt.r[:4].any() and not lt.w[:4].any() and lt.w[4].all()
    close(ph, ct, lt)
    ph, ct, lt = tables(bv, [c, list(c)], [1] * S, Y[4:], P[4:])  # the same covariate twice: the third pivot is not usable
    nul = al.Null([c, list(c)], Y[4:], P[4:])
    assert nul.fitted == [False] and nul.rounds == [1] and lt.fitted == [0] and lt.rounds == [1] and not lt.w.any()
    close(ph, ct, lt)


# ---- 2. a trait that is not 0 / 1

def test_a_value_that_is_not_0_or_1_is_refused(bv):
    S = 6
    Y = [[0, assoc.ONE, 0, assoc.ONE, 0, 0], [0, assoc.ONE, assoc.ONE // 2, 0, 2 * assoc.ONE, 0]]
    for P1, who in (([1] * S, 3), ([1, 1, 0, 1, 1, 1], 5)):
        ph = bv.PhenoTable(Y, [[1] * S, P1], names=[b"ok", b"dose"])
        with pytest.raises(bv.BvcfError) as ei:
            bv.LogitTable(ph)
        assert ei.value.rc == bv.E_ARG and "dose" in str(ei.value) and "sample %d" % who in str(ei.value)
        assert al.check_binary([b"ok", b"dose"], Y, [[1] * S, P1], list(range(1, S + 1))) == (b"dose", who)
        ph.close()
    ph = bv.PhenoTable(Y, [[1] * S, [1, 1, 0, 1, 0, 1]])  # the two values masked away: accepted
    lt = bv.LogitTable(ph)
    assert lt.n_columns == 2
    # a phenotype on a sample without covariates: the table is not the masked one
    ct = bv.CovarTable([[1, 2, 3, 4, 5, 6]], [1, 0, 1, 1, 1, 1])
    with pytest.raises(bv.BvcfError) as ei:
        bv.LogitTable(ph, ct)
    assert ei.value.rc == bv.E_ARG
    close(ph, lt, ct)


# ---- 3. operand B

# J, K and the largest |c| -> (lwc, lr, lrc, lwcc): W <= 2^22 and |R| <= 2^24 times 1, 127, 10^8, 10^12 and their squares
LIMB_CASES = [(1, 2, 1, (3, 4, 4, 3)), (2, 1, 127, (4, 4, 4, 5)), (3, 2, 10 ** 8, (7, 4, 7, 10)), (16, 1, 10 ** 12, (8, 4, 9, 13))]


@pytest.mark.parametrize("J,K,top,limbs", LIMB_CASES)
def test_operand_b(bv, J, K, top, limbs):
    rng = random.Random(9220 + J)
    S = 150
    Cv = [[top if i < 3 else -top if i < 6 else (top // 8) * rng.randint(-8, 8) if top >= 8 else rng.randint(-top, top) for i in range(S)]
          for _ in range(J)]
    complete = [0 if i == 70 else 1 for i in range(S)]
    Cv = [[c if k else 0 for c, k in zip(row, complete)] for row in Cv]
    Y = [[assoc.ONE if rng.random() < 0.45 else 0 for _ in range(S)] for _ in range(K)]
    P = [[0 if i % 11 == k else 1 for i in range(S)] for k in range(K)]
    Y, P = ac.mask(Y, P, complete)
    ph, ct, lt = tables(bv, Cv, complete, Y, P)
    nul = al.Null(Cv, Y, P)
    lay = al.layout_of(Cv, nul, P)
    assert all(nul.fitted)
    assert (lay.lwc, lay.lr, lay.lrc, lay.lwcc) == limbs
    assert (lt.lwc, lt.lr, lt.lrc, lt.lwcc, lt.n_blocks, lt.row_words, lt.s64) == limbs + (lay.n_blocks, lay.w, 192)
    B = lt.b
    want = al.operand_b(Cv, nul, P, lay)
    assert B.shape == want.shape == (16 * lay.n_blocks, 192) and (B == want).all()
    assert not B[:, S:].any() and not B[:, 70].any()  # past S; an incomplete sample
    # every value's limbs sit in one block, and the columns behind a block's values are zero
    for per, limb, first, n in ((lay.vwc, lay.lwc, 0, lay.nwc), (lay.vr, lay.lr, lay.bwc, lay.nr), (lay.vrc, lay.lrc, lay.bwc + lay.br, lay.nrc),
                                (lay.vwcc, lay.lwcc, lay.bwc + lay.br + lay.brc, lay.nwcc)):
        assert per * limb <= 16
        for blk in range(-(-n // per)):
            used = min(per, n - blk * per) * limb
            assert not B[16 * (first + blk) + used:16 * (first + blk + 1)].any()
    # the columns give the values back: sum 256^q limb
    for k in range(K):
        for i in (0, 4, 7, S - 1):
            if not P[k][i]:
                continue
            back = sum(int(B[lay.col_wcc(k, 1, J) + q][i]) << (8 * q) for q in range(lay.lwcc))
            assert back == nul.W[k][i] * Cv[0][i] * Cv[J - 1][i]
            assert sum(int(B[lay.col_r(k) + q][i]) << (8 * q) for q in range(lay.lr)) == nul.R[k][i]
    assert lt.totals.tolist() == al.totals_row(Cv, nul, P, lay)
    close(ph, ct, lt)


def test_operand_b_without_covariates(bv):
    Cv, complete, Y, P = random_case(9230, 70, 0, 3)
    ph, ct, lt = tables(bv, Cv, complete, Y, P)
    nul = al.Null(Cv, Y, P)
    lay = al.layout_of(Cv, nul, P)
    assert lay.pv == 6 and lay.bwcc == 0 and (lt.n_blocks, lt.row_words, lt.n_covars) == (lay.n_blocks, 36, 0)
    assert (lt.b == al.operand_b(Cv, nul, P, lay)).all() and lt.totals.tolist() == al.totals_row(Cv, nul, P, lay)
    close(ph, ct, lt)


# ---- 4. the statistic

def stat_cases():
    """(tag, C, complete, Y, P, (H, O, M)): random records; n = J + 2 and J + 3; a genotype that is a covariate's copy (the last
    pivot not usable) and a covariate constant on the called samples (collinear); sums past 64 bits; an unfitted phenotype"""
    out = []
    for seed, S, J, K, top in ((9240, 90, 0, 2, 1), (9241, 120, 1, 1, 3 * 10 ** 6), (9242, 150, 3, 2, 3 * 10 ** 6), (9243, 300, 16, 1, 2 * 10 ** 6)):
        Cv, complete, Y, P = random_case(seed, S, J, K, top)
        out.append(("random J=%d" % J, Cv, complete, Y, P, random_classes(random.Random(seed), 8, S)))
    # n = J + 2 and J + 3: all but a few samples missing
    Cv, complete, Y, P = random_case(9244, 80, 2, 1, na=0.0)
    cls = np.full((2, 80), 3)
    cls[0, :4] = [1, 0, 2, 1]
    cls[1, :5] = [1, 0, 2, 1, 0]
    out.append(("short", Cv, complete, Y, P, (cls == 1, cls == 2, cls == 3)))
    # g = c1 on the called samples (c1 in units: 0 / 1 / 2): d[J+1] is not usable; c2 constant where called: collinear
    rng = random.Random(9245)
    S = 60
    g = [rng.choice([0, 1, 2]) for _ in range(S)]
    c1 = [x * assoc.ONE for x in g]
    c2 = [5 * assoc.ONE if i < 40 else rng.randint(-10 ** 6, 10 ** 6) for i in range(S)]
    Y = [[assoc.ONE if rng.random() < 0.4 else 0 for _ in range(S)]]
    cls = np.array([[{0: 0, 1: 1, 2: 2}[x] for x in g], [g[i] if i < 40 else 3 for i in range(S)]])
    out.append(("unusable", [c1, [rng.randint(-10 ** 6, 10 ** 6) for _ in range(S)]], [1] * S, Y, [[1] * S], (cls[:1] == 1, cls[:1] == 2, cls[:1] == 3)))
    out.append(("collinear", [[rng.randint(-10 ** 6, 10 ** 6) for _ in range(S)], c2], [1] * S, Y, [[1] * S], (cls[1:] == 1, cls[1:] == 2, cls[1:] == 3)))
    # |c| = 10^12 and 400 samples: W C C, R C and their totals past 64 bits
    S = 400
    big = [[rng.choice([-1, 1]) * assoc.MAX_Y for _ in range(S)]]
    Y = [[assoc.ONE if rng.random() < 0.5 else 0 for _ in range(S)]]
    out.append(("wide", big, [1] * S, Y, [[1] * S], random_classes(rng, 4, S, miss=0.5)))
    # an all-1 trait beside a plain one
    Cv, complete, Y, P = random_case(9246, 100, 1, 2)
    Y[1] = [assoc.ONE if p else 0 for p in P[1]]
    out.append(("unfitted", Cv, complete, Y, P, random_classes(rng, 3, 100)))
    return out


def test_statistic_against_the_model(bv):
    seen = set()
    for tag, Cv, complete, Y, P, (H, O, M) in stat_cases():
        ph, ct, lt = tables(bv, Cv, complete, Y, P)
        nul = al.Null(Cv, Y, P)
        lay = al.layout_of(Cv, nul, P)
        J = len(Cv)
        recs, tots = assoc.records(H, O, M, Y, P), assoc.totals(Y, P)
        words = al.logit_words(H, O, M, Cv, nul, P, lay)
        tot_row = al.totals_row(Cv, nul, P, lay)
        assert lt.totals.tolist() == tot_row
        for r in range(H.shape[0]):
            for k in range(len(Y)):
                G = al.gram_of_records(words[r], tot_row, lay, k)
                direct = al.gram(H[r], O[r], M[r], Cv, nul, k, P[k])
                assert all(G[a][b] == direct[a][b] for a in range(J + 3) for b in range(min(a + 1, J + 2))), (tag, r, k)
                n, sg = tots[k][0] - recs[r][k][2], recs[r][k][0] + 2 * recs[r][k][1]
                n_, freq, st, col = al.stat(G, J, n, sg, nul.fitted[k])
                flags, out = bv.assoc_logit_stat(lt, k, recs[r][k], tots[k], words[r])
                assert flags == (freq is not None) + 2 * (st is not None) + 4 * col, (tag, r, k, flags)
                want = [float(n), freq or 0.0] + (list(st) if st else [0.0] * 4)
                assert [x.hex() for x in out] == [x.hex() for x in want], (tag, r, k)
                seen.add((tag.split(" ")[0], flags))
                if tag == "wide":
                    assert abs(G[1][1]) >= 1 << 64 and st is not None
                if tag == "short":
                    assert n == J + 2 + r and (st is not None) == (r == 1)
        close(ph, ct, lt)
    assert {("random", 3), ("short", 1), ("short", 3), ("unusable", 1), ("collinear", 5), ("wide", 3), ("unfitted", 1), ("unfitted", 3)} <= seen


def test_refusals_of_the_stat(bv):
    Cv, complete, Y, P = random_case(9250, 40, 1, 1)
    ph, ct, lt = tables(bv, Cv, complete, Y, P)
    rec, tot = (1, 1, 0, 0, 0, 0, 0), assoc.totals(Y, P)[0]
    assert bv.assoc_logit_stat(lt, 0, rec, tot, [0] * lt.row_words)[0] >= 0
    assert bv.assoc_logit_stat(lt, 1, rec, tot, [0] * lt.row_words)[0] == -1  # k >= K
    close(ph, ct, lt)


# ---- 5. and 6. what the numbers mean (CPU only)

def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def measure_meaning():
    """the largest relative deviation of the model's chisq from the unquantised doubles' over the seeds, S and J"""
    worst = 0.0
    n = 0
    for seed in al.MEANING_SEEDS:
        for S in al.MEANING_S:
            for J in al.MEANING_J:
                Cv, complete, Y, P = random_case(seed + 7 * S + J, S, J, 1, na=0.02)
                nul = al.Null(Cv, Y, P)
                assert nul.fitted == [True]
                lay = al.layout_of(Cv, nul, P)
                H, O, M = random_classes(random.Random(seed + S), 6, S, miss=0.03)
                words = al.logit_words(H, O, M, Cv, nul, P, lay)
                tot_row = al.totals_row(Cv, nul, P, lay)
                recs, tots = assoc.records(H, O, M, Y, P), assoc.totals(Y, P)
                for r in range(6):
                    st = al.stat(al.gram_of_records(words[r], tot_row, lay, 0), J, tots[0][0] - recs[r][0][2], recs[r][0][0] + 2 * recs[r][0][1], True)[2]
                    assert st is not None
                    ref = al.chisq_unquantised(H[r], O[r], M[r], Cv, Y[0], P[0], nul.beta[0])
                    if ref > 1e-3:  # (a chisq next to zero is a difference of equal sums: its relative error says nothing)
                        worst = max(worst, _rel(st[2], ref))
                        n += 1
    return worst, n


def test_meaning_against_unquantised_doubles():
    worst, n = measure_meaning()
    print("largest relative deviation of chisq from unquantised doubles: %.3e over %d statistics (bound %.3e)" % (worst, n, al.MEANING_BOUND))
    assert n > 100 and worst <= al.MEANING_BOUND


def measure_trend():
    worst = 0.0
    n = 0
    for seed in al.TREND_SEEDS:
        S = 60 + 37 * (seed % 5)
        Cv, complete, Y, P = random_case(seed, S, 0, 2)
        nul = al.Null(Cv, Y, P)
        lay = al.layout_of(Cv, nul, P)
        H, O, M = random_classes(random.Random(seed), 8, S, miss=0.0)
        # (no missing calls among the phenotype's samples: the row's sample set is the null model's)
        words = al.logit_words(H, O, M, Cv, nul, P, lay)
        tot_row = al.totals_row(Cv, nul, P, lay)
        recs, tots = assoc.records(H, O, M, Y, P), assoc.totals(Y, P)
        for r in range(8):
            for k in range(2):
                st = al.stat(al.gram_of_records(words[r], tot_row, lay, k), 0, tots[k][0], recs[r][k][0] + 2 * recs[r][k][1], nul.fitted[k])[2]
                lin = assoc.stat(recs[r][k], tots[k])[2]
                assert st is not None and lin is not None
                if lin[2] > 1e-3:
                    worst = max(worst, _rel(st[2], lin[2]))
                    n += 1
    return worst, n


def test_j0_equals_the_trend_test():
    """J = 0, no missing calls: the score test against the intercept's null model is the Cochran-Armitage trend test n r^2"""
    worst, n = measure_trend()
    print("largest relative deviation of chisq from the linear scan's: %.3e over %d statistics (bound %.3e)" % (worst, n, al.TREND_BOUND))
    assert n > 40 and worst <= al.TREND_BOUND


# ---- 8. and 9. the header, the struct, the config, the flag

def test_header_and_exports(bv):
    hdr = open(os.path.join(ROOT, "include", "bvcf.h")).read()
    for name in ("bvcf_logit_table_build", "bvcf_logit_table_free", "bvcf_set_logit_table", "bvcf_assoc_logit", "bvcf_assoc_logit_stat",
                 "bvcf_config_logit_defaults"):
        assert name + "(" in hdr and name in bv.EXPORTS
        getattr(bv.lib, name)
    assert "bvcf_bench_assoc_logit_kernels" in bv.BENCH_EXPORTS
    assert "#define BVCF_CONFIG_MORE_LOGIT 12" in hdr and bv.CONFIG_MORE_LOGIT == 12


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(bvcf_logit_table),sizeof(bvcf_assoc_logit_info),sizeof(bvcf_config_logit),offsetof(bvcf_config_logit,assoc_model),"
                   "offsetof(bvcf_logit_table,totals),sizeof(bvcf_config_covar),sizeof(bvcf_covar_table));return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [C.sizeof(bv.LogitTableStruct), C.sizeof(bv.AssocLogitInfo), C.sizeof(bv.ConfigLogit), bv.ConfigLogit.assoc_model.offset,
                   bv.LogitTableStruct.totals.offset, C.sizeof(bv.ConfigCovar), C.sizeof(bv.CovarTableStruct)]
    assert bv.ConfigLogit.assoc_model.offset == C.sizeof(bv.ConfigCovar)  # (additive: the older struct is the head, unchanged)


def test_config_markers(bv):
    c = bv.make_config({"pheno": "/p", "assoc": "/a", "covar": "/c"})
    assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_COVAR]  # (the flag off: what the twelfth marker wrote)
    c = bv.make_config({"pheno": "/p", "assoc": "/a", "covar": "/c", "assocModel": "logistic"})
    assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_LOGIT]
    v = C.cast(C.byref(c), C.POINTER(bv.ConfigLogit)).contents
    assert (v.assoc_model, v.covar.covar_path, v.covar.pca.assoc.pheno_path) == (1, b"/c", b"/p")
    c = bv.make_config({"pheno": "/p", "assoc": "/a", "assocModel": "linear"})
    v = C.cast(C.byref(c), C.POINTER(bv.ConfigLogit)).contents
    assert (v.assoc_model, v.covar.covar_path) == (0, None)
    d = bv.ConfigLogit()
    bv.lib.bvcf_config_logit_defaults(C.byref(d))
    base = d.covar.pca.assoc.score.grm.regions.variants.ld.trios.more.base
    assert list(base.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_LOGIT] and d.assoc_model == 0 and d.covar.covar_path is None
    o = bv.ConfigCovar()
    bv.lib.bvcf_config_covar_defaults(C.byref(o))
    assert list(o.pca.assoc.score.grm.regions.variants.ld.trios.more.base.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_COVAR]


def test_run_refuses_a_model_without_its_partners_or_an_unknown_one(bv):
    """bvcf_run_buffer: BVCF_E_ARG before any device work"""
    for cfg in ({"assocModel": "logistic"}, {"assocModel": 7, "pheno": "/nonexistent/p", "assoc": "/nonexistent/a"}):
        rc, out, log, _ = bv.run_buffer(vl.rows_vcf(5), cfg)
        assert rc == bv.E_ARG and out == b"" and "assoc_model" in log, (cfg, rc, log)


def cli(args, stdin_bytes=b""):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=60)


def test_cli_flag_without_a_value_its_partners_or_with_another_value():
    p = cli(["--assocModel"])
    assert p.returncode == 2 and p.stdout == b"" and p.stderr == b"flag needs an argument: -assocModel\n"
    for args in (["--assocModel="], ["--assocModel", "probit", "--pheno", "p", "--assoc", "a"], ["--assocModel", "Logistic", "--pheno", "p", "--assoc", "a"]):
        p = cli(args)
        assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1 and b"linear or logistic" in p.stderr, args
    for args in (["--assocModel", "logistic"], ["--assocModel", "linear"], ["--assocModel", "logistic", "--pheno", "p"],
                 ["--assocModel", "logistic", "--assoc", "a"], ["--assocModel", "logistic", "--covar", "c"]):
        p = cli(args, vl.rows_vcf(5))
        assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1, args


# ---- 7. the shared header under sanitizers

def fmt(x):
    return float(x).hex()


def test_arithmetic_header_alone_under_sanitizers(bv, tmp_path):
    """bvcf_assoc_logit_q.h in a program of its own: the fit, the fixed point, the layout and the statistic, bit-equal with
    the library's entry points (and so with the model)"""
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present: sanitized programs run on the build machine")
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "assoc_logit_check")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "assoc_logit_check.cpp"),
                           "-o", exe], timeout=120)
    m64 = (1 << 64) - 1
    lines, want = [], []
    for tag, Cv, complete, Y, P, (H, O, M) in stat_cases():
        ph, ct, lt = tables(bv, Cv, complete, Y, P)
        J, K, S = len(Cv), len(Y), len(P[0])
        fitted, rounds, beta = lt.fitted, lt.rounds, lt.beta
        lm, lr, lw = lt.m.tolist(), lt.r.tolist(), lt.w.tolist()
        for k in range(K):
            omega = [i for i in range(S) if P[k][i]]
            f = [J, len(omega)]
            for i in omega:
                f += [Cv[j][i] & m64 for j in range(J)] + [1 if Y[k][i] else 0]
            lines.append("fit " + " ".join(str(x) for x in f))
            w = ["fit", str(fitted[k]), str(rounds[k])] + [fmt(x) for x in beta[k]]
            if fitted[k]:
                for i in omega:
                    w += [str(lm[k][i]), str(lr[k][i]), str(lw[k][i])]
            want.append(" ".join(w))
        lay = al.Layout(J, K, lt.lwc, lt.lr, lt.lrc, lt.lwcc)
        nul = al.Null(Cv, Y, P)
        recs, tots = assoc.records(H, O, M, Y, P), assoc.totals(Y, P)
        words = al.logit_words(H, O, M, Cv, nul, P, lay)
        tot_row = lt.totals.tolist()
        n3, n2 = -(-lay.bwc // 5), -(-lay.br // 8)
        for r in range(H.shape[0]):
            for k in range(K):
                rec = recs[r][k]
                f = [J, K, lay.lwc, lay.lr, lay.lrc, lay.lwcc, k, fitted[k], rec[0], rec[1], rec[2], tots[k][0]] + words[r] + tot_row
                lines.append("stat " + " ".join(str(x) for x in f))
                flags, out = bv.assoc_logit_stat(lt, k, rec, tots[k], words[r])
                w = ["stat", lay.w, lay.n_blocks, n3, n2, n3 + n2 + -(-(lay.brc + lay.bwcc) // 16), lay.word_wc(0, 0, 0), lay.word_wc(K - 1, 2, J),
                     lay.word_r(0, 0), lay.word_r(K - 1, 1), lay.word_rc(0, 0), lay.word_rc(K - 1, J)]
                if J:
                    w += [lay.word_wcc(0, 1, 1), lay.word_wcc(K - 1, J, J)]
                want.append(" ".join([str(x) for x in w] + [str(flags)] + [fmt(x) for x in out]))
        close(ph, ct, lt)
    (tmp_path / "c.txt").write_text("".join(x + "\n" for x in lines))
    p = subprocess.run([exe, str(tmp_path / "c.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.endswith("assoc_logit_q ok\n"), out[-2000:]
    assert "ERROR" not in out and "runtime error" not in out, out[-2000:]

    def canon(line):  # (C's %a and float.hex() spell the same double differently)
        return " ".join(fmt(float.fromhex(x)) if "x" in x or x in ("inf", "-inf", "nan", "-nan") else x for x in line.split(" "))
    got = out.split("\n")[:-2]
    assert len(got) == len(want) > 60
    assert [canon(x) for x in got] == [canon(x) for x in want]
