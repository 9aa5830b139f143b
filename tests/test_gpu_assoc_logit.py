"""--assocModel logistic: the weighted sums of the logistic score test on the device (bvcf_assoc_logit.hip.h,
bvcf_set_logit_table, bvcf_assoc_logit) and the files written from the two records of a row.

The expected records and bytes come from the oracle's TSV of the same bytes (assoc_logit.py): the null fit operation for
operation in Python floats, the fixed-point vectors, class matrices of the rows' heterozygotes / homozygotes / missingGenos
lists, sums in Python integers, the elimination and the statistic operation for operation.  Every comparison is integer for
integer (the records) or byte for byte (the files): there is no tolerance."""
import gzip
import hashlib
import os
import random
import subprocess

import pytest

import assoc
import assoc_cov as ac
import assoc_logit as al
import bgzf
import grm
import gtmask
import oracle_lib as orc
import pairtable as pt
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


PATHS = {"census": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0"},
         "streaming": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "0"},
         "streaming-general": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "1"},
         "census-wide": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0", "BVCF_WIDE": "1", "BVCF_WIDE_WIN": "1000"}}


@pytest.fixture(params=list(PATHS))
def bvcf_path(request, monkeypatch):
    """every device path that leaves class maps (as in test_gpu_assoc.py)"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.fixture(params=["census", "streaming"])
def two_paths(request, monkeypatch):
    """dense maps only, and both map forms"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def streaming(monkeypatch):
    for k, v in PATHS["streaming"].items():
        monkeypatch.setenv(k, v)


def split_file(vcf):
    """-> (header fields, eol_chars, the data lines' bytes)"""
    at = vcf.index(b"#CHROM")
    end = vcf.index(b"\n", at)
    crlf = vcf[end - 1:end] == b"\r"
    return len(vcf[at:end - crlf].split(b"\t")), 2 if crlf else 1, vcf[end + 1:]


def rec_tuples(arr):
    return [[(int(r["n_het"]), int(r["n_hom"]), int(r["n_mis"]), int(r["a_het"]), int(r["a_hom"]), int(r["a_mis"]),
              (int(r["b_mis_hi"]) << 64) | int(r["b_mis_lo"])) for r in row] for row in arr]


class Tables:
    """the (masked) phenotype table and the logistic table built from it, of the files' bytes"""

    def __init__(self, bv, vcf, pheno_text, covar_text=None):
        sn = [x.encode() for x in pt.sample_names(vcf)]
        raw = bv.PhenoTable(text=pheno_text, sample_names=sn)
        if covar_text is None:
            self.pheno, self.covar = raw, None
        else:
            self.covar = bv.CovarTable(text=covar_text, sample_names=sn)
            self.pheno = raw.masked(self.covar.complete)
            raw.close()
        self.logit = bv.LogitTable(self.pheno, self.covar)

    def close(self):
        self.pheno.close()
        self.logit.close()
        if self.covar is not None:
            self.covar.close()


def ctx_records(bv, vcf, pheno_text, covar_text, allow="PASS,.", block_lines=None, **kw):
    """(the phenotypes' records, the logistic records) of a ctx that the file's data lines went through, batch after batch"""
    nh, eol, data = split_file(vcf)
    t = Tables(bv, vcf, pheno_text, covar_text)
    ctx = bv.Ctx(nh, allow=allow, eol_chars=eol, pheno=t.pheno, logit=t.logit, **kw)
    recs, words = [], []
    try:
        lines = data.split(b"\n")[:-1]
        step = block_lines or max(len(lines), 1)
        for i in range(0, len(lines), step):
            ctx.process(b"".join(x + b"\n" for x in lines[i:i + step]))
            recs += rec_tuples(ctx.assoc())
            words += ctx.assoc_logit().tolist()
        return recs, words
    finally:
        ctx.close()
        t.close()


def run_logistic(bv, vcf, pheno_text, covar_text, tmp_path, cfg=None, **kw):
    """bvcf_run_buffer with --pheno / --covar / --assoc / --assocModel logistic -> (rc, TSV body, log, output file, report)"""
    c = dict(cfg or {})
    (tmp_path / "p.tsv").write_bytes(pheno_text)
    c.update(pheno=str(tmp_path / "p.tsv"), assoc=str(tmp_path / "a.tsv"), assocReport=str(tmp_path / "a.report"), assocModel="logistic")
    if covar_text is not None:
        (tmp_path / "c.tsv").write_bytes(covar_text)
        c.update(covar=str(tmp_path / "c.tsv"))
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    return rc, out, log, (tmp_path / "a.tsv").read_bytes(), (tmp_path / "a.report").read_bytes()


def first_difference(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return "line %d: got %r want %r" % (i + 1, a, b)
    return "%d lines, want %d" % (len(g), len(w))


def words_diff(got, want):
    if len(got) != len(want):
        return "%d rows, want %d" % (len(got), len(want))
    for r, (a, b) in enumerate(zip(got, want)):
        for q, (x, y) in enumerate(zip(a, b)):
            if x != y:
                return "row %d word %d of %d: got %d want %d" % (r, q, len(b), x, y)
    return "same"


_expected = {}


def expected(key, vcf, pheno_text, covar_text, cfg=None):
    """the model's answer, computed once per input and shared by the chains"""
    if key not in _expected:
        _expected[key] = al.expected(orc.run, vcf, pheno_text, covar_text, cfg)
    return _expected[key]


def check_both(bv, key, vcf, pheno_text, covar_text, tmp_path, cfg=None, **kw):
    """raw records through a ctx and the files through bvcf_run_buffer (kw: its batch size), against the model's"""
    cfg = cfg or {}
    e = expected(key, vcf, pheno_text, covar_text, cfg)
    rc, out, log, got_out, got_rep = run_logistic(bv, vcf, pheno_text, covar_text, tmp_path, cfg, **kw)
    assert rc == 0, log
    assert out == e.body and log == e.log, "the TSV / log changed with --assocModel logistic"
    recs, words = ctx_records(bv, vcf, pheno_text, covar_text, allow=cfg.get("allow", "PASS,."), **kw)
    assert recs == e.recs, "the phenotypes' records differ"
    assert words == e.words, words_diff(words, e.words)
    assert got_rep == e.report, (got_rep, e.report)
    assert got_out == e.out, first_difference(got_out, e.out)
    return e


# ---- the kernels

@pytest.mark.parametrize("seed", [s[0] for s in pt.FUZZ])
def test_fuzz(bv, bvcf_path, tmp_path, seed):
    """J = 3, K = 2 with some NA: every row, phenotype and covariate gets different data, so a transposed C/D, a swapped class
    or a swapped pair cannot pass"""
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",", "emptyField": "NA"}
    vcf = pt.fuzz_vcf(seed)
    pheno = al.pheno_for(vcf, 2, seed, [b"T0", b"T1"] if seed % 2 else None)
    covar = ac.covar_for(vcf, 3, seed, [b"age", b"sex", b"pc1"] if seed % 2 else None, top=3 * 10 ** 6)
    e = check_both(bv, ("fuzz", seed), vcf, pheno, covar, tmp_path, cfg)
    assert len(e.recs) > 50 and e.nul.fitted[0] and e.tested > 100


@pytest.mark.parametrize("ns", grm.SAMPLE_EDGES)
def test_sample_edges(bv, two_paths, tmp_path, ns):
    """1 .. 300 samples with J = 2: a k-step short of, at and past its 64 samples, the pad bits of the last 16 map bytes (the
    smallest files leave their null models unfitted: the records are still the sums)"""
    vcf = grm.edge_vcf(ns)
    none = 0.0 if ns < 3 else 0.05
    e = check_both(bv, ("edges", ns), vcf, al.pheno_for(vcf, 2, 300 + ns, absent=none, na=none),
                   ac.covar_for(vcf, 2, 310 + ns, top=2 * 10 ** 6, absent=none, na=none), tmp_path)
    assert len(e.recs) > 20


@pytest.mark.parametrize("n_rows", assoc.DENSE_ROWS)
def test_dense_row_tile_edges(bv, monkeypatch, tmp_path, n_rows):
    """1 .. 130 dense rows with J = 3: a wave's 16 rows and a workgroup's 64 short of, at and past their edges"""
    streaming(monkeypatch)
    vcf = assoc.dense_vcf(n_rows)
    e = check_both(bv, ("dense", n_rows), vcf, al.pheno_for(vcf, 3, 400 + n_rows), ac.covar_for(vcf, 3, 410 + n_rows, top=2 * 10 ** 6), tmp_path)
    assert len(e.recs) == n_rows + 1 and e.nul.n_unfitted == 0


def test_both_map_forms(bv, bvcf_path, tmp_path):
    vcf = pt.rare_vcf(300)
    check_both(bv, "rare", vcf, al.pheno_for(vcf, 4, 610), ac.covar_for(vcf, 3, 611, top=4 * 10 ** 6), tmp_path)


def test_short_list_at_its_limit(bv, bvcf_path, tmp_path):
    """15 entries x 4 samples, missing calls among them"""
    vcf = pt.short_list_limit_vcf()
    check_both(bv, "limit", vcf, al.pheno_for(vcf, 2, 620), ac.covar_for(vcf, 2, 621, top=2 * 10 ** 6), tmp_path)


def test_min_gq_masked_calls_are_missing(bv, bvcf_path, tmp_path):
    """a third of the calls masked: the missing class carries the RC and WCC sums"""
    vcf = pt.fuzz_vcf(13)  # GT:DP:GQ, CRLF
    masked = gtmask.mask_vcf(vcf, 20, 0)
    pheno, covar = al.pheno_for(vcf, 2, 650), ac.covar_for(vcf, 3, 651, top=3 * 10 ** 6)
    e = expected("mingq", masked, pheno, covar)
    plain = expected(("fuzz-plain", 13), vcf, pheno, covar)
    assert sum(r[0][2] for r in e.recs) > sum(r[0][2] for r in plain.recs)  # more missing calls
    rc, out, log, got_out, got_rep = run_logistic(bv, vcf, pheno, covar, tmp_path, {"minGQ": 20})
    assert rc == 0, log
    assert got_rep == e.report and got_out == e.out, first_difference(got_out, e.out)


# ---- the column layout

def value_case(vcf, j, k, top, seed):
    """(phenotype file, covariate file or None): J covariates up to `top` in size, the first sample at the top, and K 0/1
    phenotypes; a covariate stays a small multiple of a unit so that the null models still fit"""
    rng = random.Random(seed)
    names = pt.sample_names(vcf)
    prow, crow = [], []
    for i, nm in enumerate(names):
        prow.append((nm.encode(), [assoc.ONE if rng.random() < 0.3 + 0.03 * c else 0 for c in range(k)]))
        crow.append((nm.encode(), [top if i == 0 else (top // 16) * rng.randint(-16, 16) for _ in range(j)]))
    return assoc.file_text(prow), ac.file_text(crow) if j else None


# J, K and the largest |C|: an intercept alone; one covariate; two phenotypes; K = 16; the maximum limb counts -- 8 / 4 / 9 / 13
# with 136 pairs, 17 + 1 + 17 + 136 blocks
COLUMN_CASES = [(0, 1, 1), (1, 1, 127), (3, 2, 10 ** 8), (2, 16, 10 ** 6), (16, 1, 10 ** 12)]


@pytest.mark.parametrize("j,k,top", COLUMN_CASES)
def test_column_layouts(bv, two_paths, tmp_path, j, k, top):
    vcf = grm.edge_vcf(130)
    pheno, covar = value_case(vcf, j, k, top, 500 + j + k)
    # (K = 16: a row's records are 5 KiB, and a run of the default batch size would pass a slot's 1 GiB -- test_ctx_above_the_cap)
    e = check_both(bv, ("columns", j, k), vcf, pheno, covar, tmp_path, max_batch_bytes=(4 << 20) if k == 16 else 0)
    t = Tables(bv, vcf, pheno, covar)
    lay = e.lay
    assert (t.logit.lwc, t.logit.lr, t.logit.lrc, t.logit.lwcc, t.logit.n_blocks, t.logit.row_words) == \
        (lay.lwc, lay.lr, lay.lrc, lay.lwcc, lay.n_blocks, lay.w)
    t.close()
    if j == 16:
        assert (lay.lwc, lay.lr, lay.lrc, lay.lwcc) == (8, 4, 9, 13) and (lay.bwc, lay.br, lay.brc, lay.bwcc) == (9, 1, 17, 136)
    if j == 0:
        assert lay.w == 2 * 6 and lay.bwcc == 0 and e.tested > 20


def test_wcc_and_rc_sums_pass_64_bits(bv, two_paths, tmp_path):
    """300 samples at C = +-10^12: in the first row all but one are missing, in the second every fourth, and those have the
    trait more often than the model says -- W C C, W C and R C summed over the missing class need the high word, R C of both
    signs"""
    vcf = assoc.big_missing_vcf()
    names = pt.sample_names(vcf)
    rng = random.Random(530)
    often = [i % 4 == 2 for i in range(len(names))]  # (the second row's missing calls)
    pheno = assoc.file_text([(nm.encode(), [assoc.ONE if rng.random() < (0.8 if o else 0.3) else 0]) for nm, o in zip(names, often)])
    covar = ac.file_text([(nm.encode(), [assoc.MAX_Y if o or rng.random() < 0.5 else -assoc.MAX_Y]) for nm, o in zip(names, often)])
    e = check_both(bv, "wide", vcf, pheno, covar, tmp_path)
    lay = e.lay
    assert e.nul.fitted == [True]
    assert al._i128(e.words[0], lay.word_wcc(0, 1, 1)) >= 1 << 64
    assert al._i128(e.words[1], lay.word_rc(0, 1)) >= 1 << 64 and al._i128(e.words[1], lay.word_wc(0, 2, 1)) >= 1 << 64
    assert any(w[q + 1] >> 63 for w in e.words for q in range(0, lay.w, 2))  # (and a negative sum: the high word all ones)


# ---- degenerate data

def test_an_unfitted_phenotype_beside_a_fitted_one(bv, two_paths, tmp_path):
    """a trait that is 1 for everybody: its null model does not fit, its records are zero and its lines print the
    --emptyField text; the phenotype beside it is tested"""
    vcf = grm.edge_vcf(65)
    pheno = al.pheno_for(vcf, 2, 700, [b"fits", b"constant"], unfitted_column=1)
    e = check_both(bv, "unfitted", vcf, pheno, ac.covar_for(vcf, 2, 701, top=2 * 10 ** 6), tmp_path, {"emptyField": "NA"})
    assert e.nul.fitted == [True, False] and e.report.endswith(b"unfitted\t1\n") and e.tested > 20
    assert all(row[1][2] is None and not row[1][3] for row in e.stats) and b"\tconstant\t" in e.out
    pv2 = 2 * e.lay.pv
    assert all(not any(w[pv2:]) for w in e.words) and any(any(w[:pv2]) for w in e.words)


def test_one_sample(bv, two_paths, tmp_path):
    vcf = grm.edge_vcf(1)
    e = check_both(bv, "one", vcf, al.pheno_for(vcf, 1, 710, na=0, absent=0), ac.covar_for(vcf, 1, 711, na=0, absent=0), tmp_path)
    assert e.tested == 0 and len(e.recs) > 0 and e.nul.n_unfitted == 1


# ---- the ctx

def test_poisoned_allocations(bv, monkeypatch, tmp_path):
    """BVCF_POISON: every fresh buffer filled with 0xa5 and held between guards -- nothing is read before it is written,
    nothing written outside its buffer"""
    monkeypatch.setenv("BVCF_POISON", "a5")
    streaming(monkeypatch)
    bv.guard_check()
    vcf = pt.rare_vcf(300)
    check_both(bv, "poison", vcf, al.pheno_for(vcf, 5, 660), ac.covar_for(vcf, 4, 661, top=3 * 10 ** 6), tmp_path)
    n, msg = bv.guard_check()
    assert n == 0, "%d buffer(s) written out of bounds, the first: %s" % (n, msg)


def test_a_logistic_table_needs_the_phenotype_table_it_was_built_from(bv):
    y, p = [[assoc.ONE, 0, assoc.ONE, 0]], [[1, 1, 1, 0]]
    ph = bv.PhenoTable(y, p)
    lt = bv.LogitTable(ph)
    other = bv.PhenoTable(y, [[1, 1, 0, 0]])
    ct = bv.CovarTable([[5, 6, 7, 8]], [1, 1, 1, 1], pheno=ph)
    for kw in (dict(logit=lt), dict(logit=lt, pheno=other), dict(logit=lt, pheno=ph, covar=ct)):
        with pytest.raises(bv.BvcfError) as ei:  # no phenotype table; built from another table; a covariate table beside it
            bv.Ctx(9 + 4, **kw)
        assert ei.value.rc == bv.E_ARG, kw
    ctx = bv.Ctx(9 + 4, pheno=ph, logit=lt)
    assert ctx.assoc_logit().shape == (0, lt.row_words)
    ctx.close()
    ctx = bv.Ctx(9 + 4, pheno=ph)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.assoc_logit()
    assert ei.value.rc == bv.E_ARG
    ctx.close()
    for t in (ph, lt, other, ct):
        t.close()


def test_ctx_above_the_cap(bv):
    """the arenas' sum past 1 GiB: one message that names the covariates, nothing allocated"""
    s = 4
    ph = bv.PhenoTable([[assoc.ONE, 0, assoc.ONE, 0]] * 2, [[1, 1, 1, 1]] * 2)
    ct = bv.CovarTable([[i + q for i in range(s)] for q in range(16)], [1] * s)
    lt = bv.LogitTable(ph, ct)
    row_bytes = 56 * 2 + 8 * lt.row_words
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + s, pheno=ph, logit=lt, max_batch_bytes=128 << 20, max_lines=1000)
    assert ei.value.rc == bv.E_TOO_BIG and "1 GiB" in str(ei.value) and "fewer covariates" in str(ei.value)
    ctx = bv.Ctx(9 + s, pheno=ph, logit=lt, max_batch_bytes=1 << 20, max_lines=1000)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.reserve_assoc_rows((1 << 30) // row_bytes + 1)
    assert ei.value.rc == bv.E_TOO_BIG and "fewer covariates" in str(ei.value)
    ctx.close()
    for t in (ph, ct, lt):
        t.close()


def test_capacity_grow_and_resubmit(bv, monkeypatch):
    """more rows than the arenas hold: the batch comes back BVCF_E_CAPACITY with the need and nothing written; after
    bvcf_reserve_assoc_rows, which grows both, the same block gives both records"""
    streaming(monkeypatch)
    vcf = assoc.many_alts_vcf()
    pheno, covar = al.pheno_for(vcf, 2, 670), ac.covar_for(vcf, 2, 671)
    e = expected("grow", vcf, pheno, covar)
    nh, eol, many = split_file(vcf)
    t = Tables(bv, vcf, pheno, covar)
    ctx = bv.Ctx(nh, eol_chars=eol, pheno=t.pheno, logit=t.logit, max_batch_bytes=64 << 10, max_lines=4000, max_alleles=8000)
    assert len(e.recs) > 512 and len(many) < 64 << 10
    ctx.submit(many)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.collect()
    assert ei.value.rc == bv.E_CAPACITY
    info = ctx.assoc_info()
    assert info.need_rows == len(e.recs) and info.n_rows == 0 and ctx.assoc_logit().shape[0] == 0
    ctx.reserve_assoc_rows(info.need_rows)
    ctx.process(many)
    recs, words = rec_tuples(ctx.assoc()), ctx.assoc_logit().tolist()
    ctx.close()
    t.close()
    assert recs == e.recs and words == e.words, words_diff(words, e.words)


def test_many_batches_two_in_flight(bv, monkeypatch):
    """batches of 40 lines through two slots: a slot's records are its own batch's"""
    streaming(monkeypatch)
    vcf = pt.rare_vcf(300)
    pheno, covar = al.pheno_for(vcf, 4, 610), ac.covar_for(vcf, 3, 611, top=4 * 10 ** 6)
    e = expected("rare", vcf, pheno, covar)
    recs, words = ctx_records(bv, vcf, pheno, covar, block_lines=40, n_slots=2)
    assert recs == e.recs and words == e.words, words_diff(words, e.words)


# ---- the CLI (each run under its own time limit)

def cli(args, stdin_bytes=None, timeout=300, env=None):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout, env=env)


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc_logit")
    vcf = vcfgen.gen_vcf(43, 1500, 200, weird=0.02) + vcfgen.gen_vcf(44, 700, 200, weird=0.02).split(b"\n", 3)[3]
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz", "pheno": d / "p.tsv", "covar": d / "c.tsv"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    # (K = 2 with J = 4 is 1.1 KB a row: the rows a default batch of a BGZF file may hold -- 671 360 at 200 samples -- stay under
    # a slot's 1 GiB; with K = 3 that run stops with the message of test_ctx_above_the_cap and wants a smaller --batchMB)
    pheno = al.pheno_for(vcf, 2, 800, names=[b"P%d" % c for c in range(2)])
    covar = ac.covar_for(vcf, 4, 801, names=[b"age", b"sex", b"pc1", b"pc2"])
    paths["pheno"].write_bytes(pheno)
    paths["covar"].write_bytes(covar)
    return vcf, paths, d, al.expected(orc.run, vcf, pheno, covar), pheno, covar


def scan_args(paths, d, tag):
    return ["--pheno", str(paths["pheno"]), "--covar", str(paths["covar"]), "--assoc", str(d / (tag + ".a")), "--assocReport", str(d / (tag + ".r")),
            "--assocModel", "logistic"]


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, e = cohort[:4]
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        p = cli(args + scan_args(paths, d, tag), stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == e.body, tag
        got = ((d / (tag + ".a")).read_bytes(), (d / (tag + ".r")).read_bytes())
        assert got[1] == e.report, (tag, got[1], e.report)
        assert got[0] == e.out, (tag, first_difference(got[0], e.out))
    assert e.tested > 1000 and e.incomplete > 0 and e.nul.n_unfitted == 0


def test_cli_the_eigenvec_of_a_pca_run_as_covariates(bv, cohort):
    """--pca P in one run, --covar P.eigenvec --assocModel logistic in the next: the "#FID IID" form as it stands"""
    vcf, paths, d, e, pheno = cohort[:5]
    p = cli(["--in", str(paths["text"]), "--noOut", "--pca", str(d / "pc"), "--pcaCount", "3"])
    assert p.returncode == 0, p.stderr[-400:]
    vec = (d / "pc.eigenvec").read_bytes()
    want = al.expected(orc.run, vcf, pheno, vec)
    p = cli(["--in", str(paths["text"]), "--noOut", "--pheno", str(paths["pheno"]), "--covar", str(d / "pc.eigenvec"), "--assoc", str(d / "pc.a"),
             "--assocReport", str(d / "pc.r"), "--assocModel", "logistic"])
    assert p.returncode == 0 and p.stdout == b"", p.stderr[-400:]
    assert want.cnames == [b"PC1", b"PC2", b"PC3"] and want.incomplete == 0 and want.tested > 1000
    assert (d / "pc.r").read_bytes() == want.report
    got = (d / "pc.a").read_bytes()
    assert got == want.out, first_difference(got, want.out)


def test_cli_other_outputs_unchanged_and_linear_is_no_flag(bv, cohort):
    vcf, paths, d, e, pheno, covar = cohort
    outs = {}
    base = ["--pheno", str(paths["pheno"]), "--covar", str(paths["covar"])]
    for tag, extra in (("plain", base + ["--assoc", str(d / "plain.a"), "--assocReport", str(d / "plain.r")]),
                       ("linear", base + ["--assoc", str(d / "linear.a"), "--assocReport", str(d / "linear.r"), "--assocModel", "linear"]),
                       ("logit", base + ["--assoc", str(d / "o.a"), "--assocModel=logistic"])):
        tsv, dos, smp, sst, prs = (d / ("%s.%s" % (tag, x)) for x in ("tsv.gz", "arrow", "samples", "stats", "pairs"))
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--compressOutput", "bgzf", "--dosageOutput", str(dos),
                 "--sample", str(smp), "--sampleStats", str(sst), "--relatedness", str(prs), "--plinkOutput", str(d / tag),
                 "--grm", str(d / tag)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        made = [tsv, dos, smp, sst, prs] + [d / (tag + x) for x in (".bed", ".bim", ".fam", ".grm.bin", ".grm.N.bin", ".grm.id")]
        outs[tag] = tuple(hashlib.sha256(f.read_bytes()).hexdigest() for f in made) + (p.stderr,)
    assert outs["plain"] == outs["logit"] == outs["linear"]
    assert (d / "o.a").read_bytes() == e.out
    # --assocModel linear and no flag: the covariate-adjusted linear scan's files, report lines included
    want = ac.expected(orc.run, vcf, pheno, covar)
    for tag in ("plain", "linear"):
        assert (d / (tag + ".a")).read_bytes() == want.out and (d / (tag + ".r")).read_bytes() == want.report, tag


def test_cli_without_covariates_a_file_without_sample_columns_and_exit_codes(bv, cohort, tmp_path):
    sites = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    vcf, paths = cohort[0], cohort[1]
    f, c = str(paths["pheno"]), str(paths["covar"])
    # J = 0: an intercept alone
    want = al.expected(orc.run, vcf, cohort[4], None)
    p = cli(["--in", str(paths["text"]), "--noOut", "--pheno", f, "--assoc", str(tmp_path / "j0.a"), "--assocReport", str(tmp_path / "j0.r"),
             "--assocModel", "logistic"])
    assert p.returncode == 0, p.stderr[-400:]
    assert (tmp_path / "j0.r").read_bytes() == want.report and want.report.endswith(b"covariates\t0\nincomplete\t0\ncollinear\t0\nunfitted\t0\n")
    got = (tmp_path / "j0.a").read_bytes()
    assert got == want.out, first_difference(got, want.out)
    # no sample columns
    p = cli(["--pheno", f, "--covar", c, "--assoc", str(tmp_path / "sites.a"), "--assocReport", str(tmp_path / "sites.r"), "--assocModel", "logistic"], sites)
    assert p.returncode == 0, p.stderr[-400:]
    assert (tmp_path / "sites.a").read_bytes() == (assoc.HEADER + "\n").encode()
    assert (tmp_path / "sites.r").read_bytes() == \
        b"columns\t2\nsamples\t0\nrows\t0\ntested\t0\ncovariates\t4\nincomplete\t0\ncollinear\t0\nunfitted\t2\n"
    # a phenotype that is not 0 / 1: one message that names the phenotype and the sample, exit code 1, the output left empty
    names = pt.sample_names(vcf)
    (tmp_path / "bad.tsv").write_bytes(assoc.file_text([(nm.encode(), [assoc.ONE, 2 * assoc.ONE if i == 5 else 0]) for i, nm in enumerate(names)],
                                                       [b"ok", b"dose"]))
    p = cli(["--pheno", str(tmp_path / "bad.tsv"), "--assoc", str(tmp_path / "bad.a"), "--assocModel", "logistic"], vcf)
    assert p.returncode == 1 and b"dose" in p.stderr and names[5].encode() in p.stderr and p.stderr.count(b"\n") == 1 and p.stdout.count(b"\n") <= 1
    assert (tmp_path / "bad.a").read_bytes() == b""
    # the flag without its partners, without a value or with another value: exit code 2
    for args in (["--assocModel", "logistic"], ["--assocModel", "logistic", "--pheno", f], ["--assocModel", "linear", "--assoc", "x"],
                 ["--assocModel"], ["--assocModel", "probit", "--pheno", f, "--assoc", "x"], ["--assocModel=", "--pheno", f, "--assoc", "x"]):
        p = cli(args, sites)
        assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1, args
