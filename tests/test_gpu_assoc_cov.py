"""--covar: the covariate sums of the association scan on the device (bvcf_assoc_cov.hip.h, bvcf_set_covar_table,
bvcf_assoc_cov) and the files written from the two records of a row.

The expected records and bytes come from the oracle's TSV of the same bytes (assoc_cov.py): class matrices of the rows'
heterozygotes / homozygotes / missingGenos lists, the values by their exact definition, sums in Python integers, the LDL^T
and the statistic operation for operation.  Every comparison is integer for integer (the records) or byte for byte (the
files): there is no tolerance."""
import gzip
import hashlib
import os
import random
import subprocess

import pytest

import assoc
import assoc_cov as ac
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
    """the masked phenotype table and the covariate table bound to it, of the two files' bytes"""

    def __init__(self, bv, vcf, pheno_text, covar_text):
        sn = [x.encode() for x in pt.sample_names(vcf)]
        raw = bv.PhenoTable(text=pheno_text, sample_names=sn)
        unbound = bv.CovarTable(text=covar_text, sample_names=sn)
        self.pheno = raw.masked(unbound.complete)
        self.covar = unbound.bound(self.pheno)
        raw.close()
        unbound.close()

    def close(self):
        self.pheno.close()
        self.covar.close()


def ctx_records(bv, vcf, pheno_text, covar_text, allow="PASS,.", block_lines=None, **kw):
    """(the phenotypes' records, the covariate records) of a ctx that the file's data lines went through, batch after batch"""
    nh, eol, data = split_file(vcf)
    t = Tables(bv, vcf, pheno_text, covar_text)
    ctx = bv.Ctx(nh, allow=allow, eol_chars=eol, pheno=t.pheno, covar=t.covar, **kw)
    recs, words = [], []
    try:
        lines = data.split(b"\n")[:-1]
        step = block_lines or max(len(lines), 1)
        for i in range(0, len(lines), step):
            ctx.process(b"".join(x + b"\n" for x in lines[i:i + step]))
            recs += rec_tuples(ctx.assoc())
            words += ctx.assoc_cov().tolist()
        return recs, words
    finally:
        ctx.close()
        t.close()


def run_with_covar(bv, vcf, pheno_text, covar_text, tmp_path, cfg=None, **kw):
    """bvcf_run_buffer with --pheno / --covar / --assoc -> (rc, TSV body, log, output file, report)"""
    c = dict(cfg or {})
    (tmp_path / "p.tsv").write_bytes(pheno_text)
    (tmp_path / "c.tsv").write_bytes(covar_text)
    c.update(pheno=str(tmp_path / "p.tsv"), covar=str(tmp_path / "c.tsv"), assoc=str(tmp_path / "a.tsv"), assocReport=str(tmp_path / "a.report"))
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
        _expected[key] = ac.expected(orc.run, vcf, pheno_text, covar_text, cfg)
    return _expected[key]


def check_both(bv, key, vcf, pheno_text, covar_text, tmp_path, cfg=None):
    """raw records through a ctx and the files through bvcf_run_buffer, against the model's"""
    cfg = cfg or {}
    e = expected(key, vcf, pheno_text, covar_text, cfg)
    rc, out, log, got_out, got_rep = run_with_covar(bv, vcf, pheno_text, covar_text, tmp_path, cfg)
    assert rc == 0, log
    assert out == e.body and log == e.log, "the TSV / log changed with --covar"
    recs, words = ctx_records(bv, vcf, pheno_text, covar_text, allow=cfg.get("allow", "PASS,."))
    assert recs == e.recs, "the phenotypes' records differ"
    assert words == e.words, words_diff(words, e.words)
    assert got_rep == e.report, (got_rep, e.report)
    assert got_out == e.out, first_difference(got_out, e.out)
    return e


# ---- the kernels

@pytest.mark.parametrize("seed", [s[0] for s in pt.FUZZ])
def test_fuzz(bv, bvcf_path, tmp_path, seed):
    """J = 3, K = 2, mixed sign and magnitude with some NA: every row, group and covariate gets different data, so a transposed
    C/D, a swapped class or a swapped pair cannot pass"""
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",", "emptyField": "NA"}
    vcf = pt.fuzz_vcf(seed)
    pheno = assoc.pheno_for(vcf, 2, seed, [b"T0", b"T1"] if seed % 2 else None, big=bool(seed & 2))
    covar = ac.covar_for(vcf, 3, seed, [b"age", b"sex", b"pc1"] if seed % 2 else None, top=10 ** 12 if seed & 2 else 3 * 10 ** 6)
    e = check_both(bv, ("fuzz", seed), vcf, pheno, covar, tmp_path, cfg)
    assert len(e.recs) > 50 and e.lay.G == 2 and e.tested > 100


@pytest.mark.parametrize("ns", grm.SAMPLE_EDGES)
def test_sample_edges(bv, two_paths, tmp_path, ns):
    """1 .. 300 samples with J = 2: a k-step short of, at and past its 64 samples, the pad bits of the last 16 map bytes"""
    vcf = grm.edge_vcf(ns)
    none = 0.0 if ns < 3 else 0.05
    e = check_both(bv, ("edges", ns), vcf, assoc.pheno_for(vcf, 2, 300 + ns, big=True, absent=none),
                   ac.covar_for(vcf, 2, 310 + ns, top=10 ** 12, absent=none, na=none), tmp_path)
    assert len(e.recs) > 20


@pytest.mark.parametrize("n_rows", assoc.DENSE_ROWS)
def test_dense_row_tile_edges(bv, monkeypatch, tmp_path, n_rows):
    """1 .. 130 dense rows with J = 3: a wave's 16 rows and a workgroup's 64 short of, at and past their edges"""
    streaming(monkeypatch)
    vcf = assoc.dense_vcf(n_rows)
    e = check_both(bv, ("dense", n_rows), vcf, assoc.pheno_for(vcf, 3, 400 + n_rows, big=True), ac.covar_for(vcf, 3, 410 + n_rows, top=10 ** 9), tmp_path)
    assert len(e.recs) == n_rows + 1


def test_both_map_forms(bv, bvcf_path, tmp_path):
    vcf = pt.rare_vcf(300)
    check_both(bv, "rare", vcf, assoc.pheno_for(vcf, 4, 610, big=True), ac.covar_for(vcf, 3, 611, top=10 ** 10), tmp_path)


def test_short_list_at_its_limit(bv, bvcf_path, tmp_path):
    """15 entries x 4 samples, missing calls among them"""
    vcf = pt.short_list_limit_vcf()
    check_both(bv, "limit", vcf, assoc.pheno_for(vcf, 2, 620, big=True), ac.covar_for(vcf, 2, 621, top=10 ** 12), tmp_path)


def test_min_gq_masked_calls_are_missing(bv, bvcf_path, tmp_path):
    """a third of the calls masked: the missing class carries the CC and CY sums"""
    vcf = pt.fuzz_vcf(13)  # GT:DP:GQ, CRLF
    masked = gtmask.mask_vcf(vcf, 20, 0)
    pheno, covar = assoc.pheno_for(vcf, 2, 650, big=True), ac.covar_for(vcf, 3, 651, top=10 ** 8)
    e = expected("mingq", masked, pheno, covar)
    plain = expected(("fuzz-plain", 13), vcf, pheno, covar)
    assert sum(r[0][2] for r in e.recs) > sum(r[0][2] for r in plain.recs)  # more missing calls
    rc, out, log, got_out, got_rep = run_with_covar(bv, vcf, pheno, covar, tmp_path, {"minGQ": 20})
    assert rc == 0, log
    assert got_rep == e.report and got_out == e.out, first_difference(got_out, e.out)


# ---- the column layout

def value_case(vcf, j, k, top, ytop, seed, patterns=None, na_at=None):
    """(phenotype file, covariate file): J covariates up to `top` and K phenotypes up to `ytop` in size, the first sample at
    the tops; patterns[c]: the samples phenotype c skips (i % 5 == patterns[c]); na_at: a sample with one NA covariate"""
    rng = random.Random(seed)
    names = pt.sample_names(vcf)
    prow, crow = [], []
    for i, nm in enumerate(names):
        ys = [ytop if i == 0 else rng.randint(-ytop, ytop) for _ in range(k)]
        if patterns:
            ys = [None if i and i % 5 == patterns[c] else y for c, y in enumerate(ys)]
        cs = [top if i == 0 else rng.randint(-top, top) for _ in range(j)]
        if i == na_at:
            cs[-1] = None
        prow.append((nm.encode(), ys))
        crow.append((nm.encode(), cs))
    return assoc.file_text(prow), ac.file_text(crow)


# J, K, the largest |C| and |Y| -> (lc, lcc, lcy), the blocks' slices: one limb; 6 / 11 / 11 limbs with 136 products -- 8 + 136
# + 16 blocks in 2 + 10 slices; seven limbs -- two values and two zero columns a block; K = 16
COLUMN_CASES = [(1, 1, 127, 1, (1, 2, 1)), (16, 1, 10 ** 12, 10 ** 12, (6, 11, 11)), (2, 2, 10 ** 8, 10 ** 8, (4, 7, 7)),
                (2, 16, 1000, 10 ** 6, (2, 3, 4))]


@pytest.mark.parametrize("j,k,top,ytop,limbs", COLUMN_CASES)
def test_column_layouts(bv, two_paths, tmp_path, j, k, top, ytop, limbs):
    vcf = grm.edge_vcf(65)
    pheno, covar = value_case(vcf, j, k, top, ytop, 500 + j + k)
    e = check_both(bv, ("columns", j, k), vcf, pheno, covar, tmp_path)
    assert (e.lay.lc, e.lay.lcc, e.lay.lcy) == limbs
    t = Tables(bv, vcf, pheno, covar)
    assert (t.covar.lc, t.covar.lcc, t.covar.lcy, t.covar.n_blocks, t.covar.row_words) == limbs + (e.lay.n_blocks, e.lay.w)
    t.close()
    if j == 16:
        assert e.lay.np2 == 136 and (e.lay.bc, e.lay.bcc, e.lay.bcy) == (8, 136, 16) and e.tested > 20


def test_two_mask_groups_and_an_incomplete_sample(bv, two_paths, tmp_path):
    """K = 3 with the presence patterns A, A, B and one NA covariate: two groups, one incomplete sample"""
    vcf = grm.edge_vcf(65)
    pheno, covar = value_case(vcf, 2, 3, 10 ** 7, 10 ** 7, 520, patterns=[1, 1, 2], na_at=7)
    e = check_both(bv, "groups", vcf, pheno, covar, tmp_path)
    assert e.group_of == [0, 0, 1] and e.incomplete == 1 and e.report.endswith(b"covariates\t2\nincomplete\t1\ncollinear\t0\n")
    assert e.tots[0][0] == e.tots[1][0] == 65 - 13 - 1 and e.P[0][7] == 0


def test_cc_and_cy_sums_pass_64_bits(bv, two_paths, tmp_path):
    """300 samples at C = +-10^12 and Y = -10^12, all but one missing in a row: the sums need the high word, of both signs"""
    vcf = assoc.big_missing_vcf()
    names = pt.sample_names(vcf)
    pheno = assoc.file_text([(nm.encode(), [-assoc.MAX_Y]) for nm in names])
    covar = ac.file_text([(nm.encode(), [assoc.MAX_Y, -assoc.MAX_Y]) for nm in names])
    e = check_both(bv, "wide", vcf, pheno, covar, tmp_path)
    lay = e.lay
    assert e.words[0][lay.word_cc(0, 0, 0)] + (e.words[0][lay.word_cc(0, 0, 0) + 1] << 64) == 299 * 10 ** 24 >= 1 << 64
    assert e.words[0][lay.word_cc(0, 0, 1) + 1] >> 63 and e.words[0][lay.word_cy(0, 0) + 1] >> 63  # negative sums
    assert e.collinear > 0  # (c2 = -c1)


# ---- degenerate data

def test_collinear_constant_and_short_data(bv, two_paths, tmp_path):
    """c2 = 2 c1 and a constant covariate print the --emptyField text and count as collinear; n < J + 3; a phenotype nobody
    has"""
    vcf = grm.edge_vcf(65)
    rng = random.Random(700)
    names = pt.sample_names(vcf)
    pheno = assoc.file_text([(nm.encode(), [rng.randint(-10 ** 7, 10 ** 7), None]) for nm in names], [b"y", b"nobody"])
    c1 = [rng.randint(-10 ** 7, 10 ** 7) for _ in names]
    e = check_both(bv, "c2=2c1", vcf, pheno, ac.file_text([(nm.encode(), [c, 2 * c]) for nm, c in zip(names, c1)]), tmp_path,
                   {"emptyField": "NA"})
    n_big = sum(1 for row in e.stats if row[0][0] >= 5)
    assert e.tested == 0 and e.collinear == n_big > 20 and b"\tNA\tNA\tNA\tNA\n" in e.out
    assert all(row[1][0] == 0 and row[1][1] is None for row in e.stats)  # the phenotype nobody has: n = 0
    e = check_both(bv, "constant", vcf, pheno, ac.file_text([(nm.encode(), [c, 5 * 10 ** 6]) for nm, c in zip(names, c1)]), tmp_path)
    assert e.tested == 0 and e.collinear > 20
    # five samples with J = 3: n < J + 3 everywhere
    vcf = grm.edge_vcf(5)
    e = check_both(bv, "short", vcf, assoc.pheno_for(vcf, 1, 701, na=0, absent=0), ac.covar_for(vcf, 3, 702, na=0, absent=0), tmp_path)
    assert e.tested == 0 and e.collinear == 0 and len(e.recs) > 0


def test_one_sample(bv, two_paths, tmp_path):
    vcf = grm.edge_vcf(1)
    e = check_both(bv, "one", vcf, assoc.pheno_for(vcf, 1, 710, na=0, absent=0), ac.covar_for(vcf, 1, 711, na=0, absent=0), tmp_path)
    assert e.tested == 0 and len(e.recs) > 0


# ---- the ctx

def test_poisoned_allocations(bv, monkeypatch, tmp_path):
    """BVCF_POISON: every fresh buffer filled with 0xa5 and held between guards -- nothing is read before it is written,
    nothing written outside its buffer"""
    monkeypatch.setenv("BVCF_POISON", "a5")
    streaming(monkeypatch)
    bv.guard_check()
    vcf = pt.rare_vcf(300)
    check_both(bv, "poison", vcf, assoc.pheno_for(vcf, 5, 660, big=True), ac.covar_for(vcf, 4, 661, top=10 ** 11), tmp_path)
    n, msg = bv.guard_check()
    assert n == 0, "%d buffer(s) written out of bounds, the first: %s" % (n, msg)


def test_a_covariate_table_needs_the_phenotype_table_it_is_bound_to(bv):
    y, p = [[1, 2, 3, 4]], [[1, 1, 1, 0]]
    ph = bv.PhenoTable(y, p)
    ct = bv.CovarTable([[5, 6, 7, 8]], [1, 1, 1, 1], pheno=ph)
    unbound = bv.CovarTable([[5, 6, 7, 8]], [1, 1, 1, 1])
    other = bv.PhenoTable(y, [[1, 1, 0, 0]])
    for kw in (dict(covar=ct), dict(covar=unbound, pheno=ph), dict(covar=ct, pheno=other)):
        with pytest.raises(bv.BvcfError) as ei:  # no phenotype table; an unbound table; bound to another table
            bv.Ctx(9 + 4, **kw)
        assert ei.value.rc == bv.E_ARG, kw
    ctx = bv.Ctx(9 + 4, pheno=ph, covar=ct)
    assert ctx.assoc_cov().shape == (0, ct.row_words)
    ctx.close()
    ctx = bv.Ctx(9 + 4, pheno=ph)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.assoc_cov()
    assert ei.value.rc == bv.E_ARG
    ctx.close()
    for t in (ph, ct, unbound, other):
        t.close()


def test_ctx_above_the_cap(bv):
    """the two arenas' sum past 1 GiB: one message that names the covariates, nothing allocated"""
    s = 4
    ph = bv.PhenoTable([[1, 2, 3, 4]] * 2, [[1, 1, 1, 1]] * 2)
    ct = bv.CovarTable([[i + q for i in range(s)] for q in range(16)], [1] * s, pheno=ph)
    row_bytes = 56 * 2 + 8 * ct.row_words
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + s, pheno=ph, covar=ct, max_batch_bytes=128 << 20, max_lines=1000)
    assert ei.value.rc == bv.E_TOO_BIG and "1 GiB" in str(ei.value) and "fewer covariates" in str(ei.value)
    ctx = bv.Ctx(9 + s, pheno=ph, covar=ct, max_batch_bytes=1 << 20, max_lines=1000)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.reserve_assoc_rows((1 << 30) // row_bytes + 1)
    assert ei.value.rc == bv.E_TOO_BIG and "fewer covariates" in str(ei.value)
    ctx.close()
    ph.close()
    ct.close()


def test_capacity_grow_and_resubmit(bv, monkeypatch):
    """more rows than the arenas hold: the batch comes back BVCF_E_CAPACITY with the need and nothing written; after
    bvcf_reserve_assoc_rows, which grows both, the same block gives both records"""
    streaming(monkeypatch)
    vcf = assoc.many_alts_vcf()
    pheno, covar = assoc.pheno_for(vcf, 2, 670), ac.covar_for(vcf, 2, 671)
    e = expected("grow", vcf, pheno, covar)
    nh, eol, many = split_file(vcf)
    t = Tables(bv, vcf, pheno, covar)
    ctx = bv.Ctx(nh, eol_chars=eol, pheno=t.pheno, covar=t.covar, max_batch_bytes=64 << 10, max_lines=4000, max_alleles=8000)
    assert len(e.recs) > 512 and len(many) < 64 << 10
    ctx.submit(many)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.collect()
    assert ei.value.rc == bv.E_CAPACITY
    info = ctx.assoc_info()
    assert info.need_rows == len(e.recs) and info.n_rows == 0 and ctx.assoc_cov().shape[0] == 0
    ctx.reserve_assoc_rows(info.need_rows)
    ctx.process(many)
    recs, words = rec_tuples(ctx.assoc()), ctx.assoc_cov().tolist()
    ctx.close()
    t.close()
    assert recs == e.recs and words == e.words, words_diff(words, e.words)


def test_many_batches_two_in_flight(bv, monkeypatch):
    """batches of 40 lines through two slots: a slot's records are its own batch's"""
    streaming(monkeypatch)
    vcf = pt.rare_vcf(300)
    pheno, covar = assoc.pheno_for(vcf, 4, 610, big=True), ac.covar_for(vcf, 3, 611, top=10 ** 10)
    e = expected("rare", vcf, pheno, covar)
    recs, words = ctx_records(bv, vcf, pheno, covar, block_lines=40, n_slots=2)
    assert recs == e.recs and words == e.words, words_diff(words, e.words)


# ---- the CLI (each run under its own time limit)

def cli(args, stdin_bytes=None, timeout=300, env=None):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout, env=env)


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc_cov")
    vcf = vcfgen.gen_vcf(43, 1500, 200, weird=0.02) + vcfgen.gen_vcf(44, 700, 200, weird=0.02).split(b"\n", 3)[3]
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz", "pheno": d / "p.tsv", "covar": d / "c.tsv"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    pheno = assoc.pheno_for(vcf, 3, 800, names=[b"P%d" % c for c in range(3)], binary_column=1)
    covar = ac.covar_for(vcf, 4, 801, names=[b"age", b"sex", b"pc1", b"pc2"])
    paths["pheno"].write_bytes(pheno)
    paths["covar"].write_bytes(covar)
    return vcf, paths, d, ac.expected(orc.run, vcf, pheno, covar), pheno


def scan_args(paths, d, tag):
    return ["--pheno", str(paths["pheno"]), "--covar", str(paths["covar"]), "--assoc", str(d / (tag + ".a")), "--assocReport", str(d / (tag + ".r"))]


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, e, _ = cohort
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
    assert e.tested > 1000 and e.incomplete > 0


def test_cli_the_eigenvec_of_a_pca_run_as_covariates(bv, cohort):
    """--pca P in one run, --covar P.eigenvec in the next: the "#FID IID" form as it stands"""
    vcf, paths, d, e, pheno = cohort
    p = cli(["--in", str(paths["text"]), "--noOut", "--pca", str(d / "pc"), "--pcaCount", "3"])
    assert p.returncode == 0, p.stderr[-400:]
    vec = (d / "pc.eigenvec").read_bytes()
    assert vec.startswith(b"#FID\tIID\tPC1\tPC2\tPC3\n")
    want = ac.expected(orc.run, vcf, pheno, vec)
    p = cli(["--in", str(paths["text"]), "--noOut", "--pheno", str(paths["pheno"]), "--covar", str(d / "pc.eigenvec"), "--assoc", str(d / "pc.a"),
             "--assocReport", str(d / "pc.r")])
    assert p.returncode == 0 and p.stdout == b"", p.stderr[-400:]
    assert want.cnames == [b"PC1", b"PC2", b"PC3"] and want.incomplete == 0 and want.tested > 1000
    assert (d / "pc.r").read_bytes() == want.report
    got = (d / "pc.a").read_bytes()
    assert got == want.out, first_difference(got, want.out)


def test_cli_other_outputs_unchanged_and_no_flag_no_change(bv, cohort):
    vcf, paths, d, e, pheno = cohort
    outs = {}
    base = ["--pheno", str(paths["pheno"])]
    for tag, extra in (("plain", base + ["--assoc", str(d / "plain.a"), "--assocReport", str(d / "plain.r")]),
                       ("covar", base + ["--covar", str(paths["covar"]), "--assoc", str(d / "o.a")])):
        tsv, dos, smp, sst, prs = (d / ("%s.%s" % (tag, x)) for x in ("tsv.gz", "arrow", "samples", "stats", "pairs"))
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--compressOutput", "bgzf", "--dosageOutput", str(dos),
                 "--sample", str(smp), "--sampleStats", str(sst), "--relatedness", str(prs), "--plinkOutput", str(d / tag),
                 "--grm", str(d / tag)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        made = [tsv, dos, smp, sst, prs] + [d / (tag + x) for x in (".bed", ".bim", ".fam", ".grm.bin", ".grm.N.bin", ".grm.id")]
        outs[tag] = tuple(hashlib.sha256(f.read_bytes()).hexdigest() for f in made) + (p.stderr,)
    assert outs["plain"] == outs["covar"]
    assert (d / "o.a").read_bytes() == e.out
    # without --covar the scan's files are the unadjusted model's, report lines included
    want = assoc.expected(orc.run, vcf, pheno)
    assert (d / "plain.a").read_bytes() == want[2] and (d / "plain.r").read_bytes() == want[3]


def test_cli_a_file_without_sample_columns_and_exit_codes(bv, cohort, tmp_path):
    sites = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    vcf, paths = cohort[0], cohort[1]
    f, c = str(paths["pheno"]), str(paths["covar"])
    p = cli(["--pheno", f, "--covar", c, "--assoc", str(tmp_path / "sites.a"), "--assocReport", str(tmp_path / "sites.r")], sites)
    assert p.returncode == 0, p.stderr[-400:]
    assert (tmp_path / "sites.a").read_bytes() == (assoc.HEADER + "\n").encode()
    assert (tmp_path / "sites.r").read_bytes() == b"columns\t3\nsamples\t0\nrows\t0\ntested\t0\ncovariates\t4\nincomplete\t0\ncollinear\t0\n"
    # a bad covariate file and an unreadable one: one message that names the line, exit code 1, the output left empty
    (tmp_path / "bad.tsv").write_bytes(b"#sample\ta\nS1\t1\nS2\tx\n")
    p = cli(["--pheno", f, "--covar", str(tmp_path / "bad.tsv"), "--assoc", str(tmp_path / "bad.a")], vcf)
    assert p.returncode == 1 and b"covar:" in p.stderr and b"line 3:" in p.stderr and p.stderr.count(b"\n") == 1 and p.stdout.count(b"\n") <= 1
    assert (tmp_path / "bad.a").read_bytes() == b""
    p = cli(["--pheno", f, "--covar", str(tmp_path / "none.tsv"), "--assoc", str(tmp_path / "none.a")], vcf)
    assert p.returncode == 1 and b"none.tsv" in p.stderr and p.stderr.count(b"\n") == 1 and p.stdout.count(b"\n") <= 1
    # the flag without its partners or without a value: exit code 2
    for args in (["--covar", c], ["--covar", c, "--pheno", f], ["--covar", c, "--assoc", "x"], ["--covar"]):
        p = cli(args, sites)
        assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1
