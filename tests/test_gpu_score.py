"""--score: the per-sample scores summed on the device (bvcf_score.hip.h, bvcf_set_score_table, bvcf_score) and the files
written from them.

The expected words and bytes come from the oracle's TSV of the same bytes (score.py): dosage matrices of the rows'
heterozygotes / homozygotes / missingGenos lists, the weights by their exact definition, products in Python integers.
Every comparison is byte for byte (the files) or integer for integer (the words): there is no tolerance."""
import gzip
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf
import grm
import gtmask
import oracle_lib as orc
import pairtable as pt
import regions as rg
import samplecut
import score
import sitegate as sg
import variantlist as vl
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")
NOWHERE = [b"chr9:1:A:T", b"chr1:100:A:TT", b"1:100:A:T"]  # entries no row matches


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
    """every device path that leaves class maps (as in test_gpu_grm.py)"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.fixture(params=["census", "streaming"])
def two_paths(request, monkeypatch):
    """dense maps only, and both map forms"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def split_file(vcf):
    """-> (header fields, eol_chars, the data lines' bytes)"""
    at = vcf.index(b"#CHROM")
    end = vcf.index(b"\n", at)
    crlf = vcf[end - 1:end] == b"\r"
    return len(vcf[at:end - crlf].split(b"\t")), 2 if crlf else 1, vcf[end + 1:]


def ctx_scores(bv, vcf, score_text, allow="PASS,.", block_lines=None, **kw):
    """(T, G, X, R) of a ctx that the file's data lines went through"""
    nh, eol, data = split_file(vcf)
    table = bv.ScoreTable(text=score_text)
    ctx = bv.Ctx(nh, allow=allow, eol_chars=eol, score=table, **kw)
    try:
        if block_lines is None:
            ctx.process(data)
        else:
            lines = data.split(b"\n")[:-1]
            for i in range(0, len(lines), block_lines):
                ctx.process(b"".join(x + b"\n" for x in lines[i:i + block_lines]))
        return ctx.scores()
    finally:
        ctx.close()
        table.close()


def run_with_score(bv, vcf, score_text, tmp_path, cfg=None, **kw):
    """bvcf_run_buffer with --score -> (rc, TSV body, log, output file, report)"""
    c = dict(cfg or {})
    (tmp_path / "w.tsv").write_bytes(score_text)
    c.update(score=str(tmp_path / "w.tsv"), scoreOutput=str(tmp_path / "s.tsv"), scoreReport=str(tmp_path / "s.report"))
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    return rc, out, log, (tmp_path / "s.tsv").read_bytes(), (tmp_path / "s.report").read_bytes()


def sums_diff(got, want):
    (T, G, X, R), (Tw, Gw, Xw, Rw) = got, want
    if R != Rw:
        return "R: got %d want %d" % (R, Rw)
    for name, a, b in (("G", G, Gw), ("X", X, Xw)):
        if list(a) != list(b):
            i = [x != y for x, y in zip(a, b)].index(True) if len(a) == len(b) else -1
            return "%s: sample %d: got %s want %s" % (name, i, a[i] if i >= 0 else len(a), b[i] if i >= 0 else len(b))
    for i, (row, roww) in enumerate(zip(T, Tw)):
        for c, (a, b) in enumerate(zip(row, roww)):
            if a != b:
                return "T[%d][%d]: got %d want %d (difference %d)" % (i, c, a, b, a - b)
    return "shape: %d x ?, want %d x ?" % (len(T), len(Tw))


def same_sums(got, want):
    return (got[3] == want[3] and list(got[1]) == list(want[1]) and list(got[2]) == list(want[2]) and
            [list(r) for r in got[0]] == [list(r) for r in want[0]])


_BODY = {}


def oracle_body(vcf, cfg=None):
    cfg = cfg or {}
    key = (hashlib.sha256(vcf).digest(), tuple(sorted(cfg.items())))
    if key not in _BODY:
        rc, body, log, _ = orc.run(vcf, cfg)
        assert rc == 0
        _BODY[key] = (body, log)
    return _BODY[key]


def make_text(vcf, k, seed, cfg=None, names=None, **kw):
    """a score file over the loci of the file's rows (score.entries_for) plus entries that match nothing"""
    loci = vl.loci_of(oracle_body(vcf, cfg)[0])
    kw.setdefault("extra", NOWHERE)
    return score.file_text(score.entries_for(loci, k, seed, **kw), names)


def check_both(bv, vcf, score_text, tmp_path, cfg=None):
    """raw words through a ctx and the files through bvcf_run_buffer, against the oracle's"""
    cfg = cfg or {}
    want, want_out, want_rep, out_o, log_o = score.expected(orc.run, vcf, score_text, cfg)
    rc, out, log, got_out, got_rep = run_with_score(bv, vcf, score_text, tmp_path, cfg)
    assert rc == 0, log
    assert out == out_o and log == log_o, "the TSV / log changed with --score"
    got = ctx_scores(bv, vcf, score_text, allow=cfg.get("allow", "PASS,."))
    assert same_sums(got, want), sums_diff(got, want)
    assert got_rep == want_rep, (got_rep, want_rep)
    assert got_out == want_out, first_difference(got_out, want_out)
    return want


def first_difference(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            fa, fb = a.split(b"\t"), b.split(b"\t")
            for c, (x, y) in enumerate(zip(fa, fb)):
                if x != y:
                    return "line %d field %d: got %r want %r" % (i + 1, c, x, y)
            return "line %d: %d fields, want %d" % (i + 1, len(fa), len(fb))
    return "%d lines, want %d" % (len(g), len(w))


# ---- table cases

@pytest.mark.parametrize("seed", [s[0] for s in pt.FUZZ])
def test_fuzz(bv, bvcf_path, tmp_path, seed):
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",",
                                          "emptyField": "NA"}
    vcf = pt.fuzz_vcf(seed)
    names = [b"PGS%d" % c for c in range(3)] if seed % 2 else None
    R = check_both(bv, vcf, make_text(vcf, 3, seed, cfg, names, big=bool(seed & 2), frac=0.6), tmp_path, cfg)[3]
    assert R > 50


@pytest.mark.parametrize("ns", grm.SAMPLE_EDGES)
def test_sample_edges(bv, two_paths, tmp_path, ns):
    """1 .. 300 samples: an MFMA block short of, at and past 16 samples, a workgroup's block likewise at 64, five blocks at
    300.  Two columns of mixed signs and eight limbs: a transposed C/D write or a mis-weighted limb cannot pass"""
    vcf = grm.edge_vcf(ns)
    T = check_both(bv, vcf, make_text(vcf, 2, 300 + ns, big=True), tmp_path)[0]
    assert any(t[0] != t[1] for t in T) and (ns == 1 or len({tuple(t) for t in T}) > 1)


@pytest.mark.parametrize("n_rows", pt.TILE_ROWS)
def test_row_tile_edges(bv, monkeypatch, tmp_path, n_rows):
    """1, 63, 64, 65 and 130 matched dense rows: a k-step short of, at and past its 64 rows"""
    for k, v in PATHS["census"].items():
        monkeypatch.setenv(k, v)
    vcf = pt.tile_vcf(n_rows)
    assert check_both(bv, vcf, make_text(vcf, 3, 400 + n_rows, big=True), tmp_path)[3] == n_rows


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("k", score.COLUMN_EDGES)
def test_column_edges(bv, two_paths, tmp_path, k, big):
    """K = 1, 15, 16, 17, 64 with L = 1 (every |W| <= 127) and L = 8 (+-10^18 beside +-1): the constant column falls in the
    first 16-column block, starts a block of its own, and the columns pass a workgroup's 128"""
    vcf = grm.edge_vcf(65)
    text = make_text(vcf, k, 500 + k, big=big)
    table = bv.ScoreTable(text=text)
    assert (table.n_columns, table.n_limbs) == (k, 8 if big else 1)
    table.close()
    check_both(bv, vcf, text, tmp_path)


def test_a_column_of_weights_that_quantise_to_zero(bv, two_paths, tmp_path):
    vcf = pt.rare_vcf(129)
    T = check_both(bv, vcf, make_text(vcf, 3, 600, zero_column=1), tmp_path)[0]
    assert not any(t[1] for t in T) and any(t[0] for t in T) and any(t[2] for t in T)


def test_both_map_forms_are_matched(bv, bvcf_path, tmp_path):
    check_both(bv, pt.rare_vcf(300), make_text(pt.rare_vcf(300), 4, 610, big=True, frac=0.7), tmp_path)


def test_short_list_at_its_limit(bv, bvcf_path, tmp_path):
    """15 entries x 4 samples, missing calls among them"""
    vcf = pt.short_list_limit_vcf()
    check_both(bv, vcf, make_text(vcf, 2, 620, big=True), tmp_path)


def test_half_missing_and_all_missing_samples(bv, bvcf_path, tmp_path):
    vcf = pt.half_missing_vcf()
    check_both(bv, vcf, make_text(vcf, 2, 630), tmp_path)
    vcf = grm.all_missing_sample_vcf()
    T, G, X, R = check_both(bv, vcf, make_text(vcf, 2, 631), tmp_path)
    assert R > 0 and X[2] == R  # sample 2 is never called: its AVG is the empty field


def test_all_hom_rows_count(bv, bvcf_path, tmp_path):
    """monomorphic rows are not skipped: an all-hom row adds 2 W to everyone"""
    vcf = score.all_hom_vcf()
    loci = vl.loci_of(oracle_body(vcf)[0])
    text = score.file_text([(loci[0], [7, -3]), (loci[3], [10 ** 18, 1])])
    T, G, X, R = check_both(bv, vcf, text, tmp_path)
    assert R == 2 and T[0] == [14 + 2 * 10 ** 18, -6 + 2] and G[0] == 4


def test_multiallelic_lines_and_a_locus_on_two_lines(bv, bvcf_path, tmp_path):
    vcf = score.multiallelic_vcf()
    assert check_both(bv, vcf, make_text(vcf, 2, 640, big=True), tmp_path)[3] > 40
    vcf = score.twice_vcf()
    assert check_both(bv, vcf, make_text(vcf, 2, 641), tmp_path)[3] == 4


def test_entries_that_match_nothing_and_a_header_alone(bv, two_paths, tmp_path):
    vcf = pt.tile_vcf(65)
    T, G, X, R = check_both(bv, vcf, score.file_text([(x, [5, -5]) for x in NOWHERE]), tmp_path)
    assert R == 0 and not any(G) and not any(X)
    (tmp_path / "h").mkdir()
    T, G, X, R = check_both(bv, vcf, b"#locus\tA\tB\r\n", tmp_path / "h")
    assert R == 0 and T[0] == [0, 0]


def test_sums_pass_64_bits(bv, monkeypatch):
    """150 000 identical all-hom rows at W = 10^18 in ONE batch: T = 3 * 10^23 needs the high word"""
    for k, v in PATHS["census"].items():
        monkeypatch.setenv(k, v)
    n = score.FLUSH_ROWS
    text = score.file_text([(b"chr3:100:C:T", [10 ** 18, -10 ** 18, 1])])
    got = ctx_scores(bv, score.flush_vcf(), text, max_batch_bytes=16 << 20, max_lines=n + 100, max_alleles=n + 200)
    assert 2 * n * 10 ** 18 >= 1 << 64
    want = ([[2 * n * 10 ** 18, -2 * n * 10 ** 18, 2 * n]] * 8, [2 * n] * 8, [0] * 8, n)
    assert same_sums(got, want), sums_diff(got, want)


def test_min_gq_masked_calls_are_missing(bv, bvcf_path, tmp_path):
    vcf = pt.fuzz_vcf(13)  # GT:DP:GQ, CRLF
    masked = gtmask.mask_vcf(vcf, 20, 0)
    text = make_text(masked, 2, 650, big=True)
    want, want_out, want_rep, _, _ = score.expected(orc.run, masked, text)
    assert sum(want[2]) > sum(score.expected(orc.run, vcf, text)[0][2])  # more missing calls
    rc, out, log, got_out, got_rep = run_with_score(bv, vcf, text, tmp_path, {"minGQ": 20})
    assert rc == 0, log
    assert got_rep == want_rep and got_out == want_out, first_difference(got_out, want_out)


def test_poisoned_allocations(bv, monkeypatch, tmp_path):
    """BVCF_POISON: every fresh buffer filled with 0xa5 and held between guards -- nothing is read before it is written,
    nothing written outside its buffer"""
    monkeypatch.setenv("BVCF_POISON", "a5")
    for k, v in PATHS["streaming"].items():
        monkeypatch.setenv(k, v)
    bv.guard_check()
    vcf = pt.rare_vcf(300)
    check_both(bv, vcf, make_text(vcf, 17, 660, big=True), tmp_path)
    n, msg = bv.guard_check()
    assert n == 0, "%d buffer(s) written out of bounds, the first: %s" % (n, msg)


# ---- the Ctx

def test_ctx_without_a_table_and_without_samples(bv):
    ctx = bv.Ctx(9 + 4)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.score_words()
    assert ei.value.rc == bv.E_ARG
    ctx.close()
    table = bv.ScoreTable([b"chr1:1:A:T"], [[1, 2]])
    ctx = bv.Ctx(9, score=table)  # no sample columns: a no-op, and no sample's words
    lo, hi, g, x, r = ctx.score_words()
    assert lo.shape == (0, 2) and r == 0
    ctx.close()
    table.close()


def test_ctx_above_the_cap(bv):
    """a slot's tables past 1 GiB: one message, nothing allocated"""
    table = bv.ScoreTable([b"chr1:1:A:T"], [[10 ** 18] * 64])
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + 300000, score=table, max_batch_bytes=4 << 20, max_lines=1000)
    assert ei.value.rc == bv.E_TOO_BIG and "1 GiB" in str(ei.value)
    table.close()


# ---- the 1KG slice: 2 504 samples, 40 sample blocks

@pytest.fixture(scope="module")
def golden(golden_1kg):
    """the slice's TSV body and dosage matrices through the oracle, once, with scores on a seeded tenth of its loci"""
    vcf = golden_1kg[0]
    rc, body, _, _ = orc.run(vcf)
    assert rc == 0
    names = pt.sample_names(vcf)
    H, O, M = pt.matrices(body, names)
    for x in (H, O, M):
        x.setflags(write=False)
    loci = vl.loci_of(body)
    cols = [b"PGS000001", b"PC1", b"PC2", b"PC3"]
    entries = score.entries_for(loci, 4, 700, big=True, frac=0.1, extra=NOWHERE)
    return vcf, body, names, (H, O, M), loci, cols, entries, score.file_text(entries, cols)


def golden_files(golden, mask=None, cols=None):
    """the words and the output file of the slice's rows that stay (mask) over the samples that stay (cols; a row no kept
    sample carries is no row)"""
    vcf, body, names, (H, O, M), loci, colnames, entries, text = golden
    if mask is not None:
        keep = np.asarray(mask, dtype=bool)
        H, O, M = H[keep], O[keep], M[keep]
        loci = [x for x, m in zip(loci, keep) if m]
    if cols is not None:
        H, O, M = H[:, cols], O[:, cols], M[:, cols]
        rows = (H.sum(axis=1) + O.sum(axis=1)) > 0
        H, O, M = H[rows], O[rows], M[rows]
        loci = [x for x, m in zip(loci, rows) if m]
        names = [names[c] for c in cols]
    t = score.sums_m(H, O, M, loci, entries, 4)
    return t, score.output_text(*t, names, colnames)


@pytest.fixture(scope="module")
def golden_full(golden):
    return golden_files(golden)


def cli(args, stdin_bytes=None, timeout=300, env=None):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout, env=env)


def add(a, b):
    return ([[x + y for x, y in zip(r, s)] for r, s in zip(a[0], b[0])], [x + y for x, y in zip(a[1], b[1])],
            [x + y for x, y in zip(a[2], b[2])], a[3] + b[3])


def test_golden_many_batches_and_a_reset(bv, golden, golden_full, monkeypatch):
    """the slice in batches of 1 500 lines, two in flight, maps made on the device only; the totals are read and reset half
    way: the two readings add up to the whole"""
    monkeypatch.setenv("BVCF_PATH", "2")
    vcf = golden[0]
    nh, eol, data = split_file(vcf)
    lines = data.split(b"\n")[:-1]
    blocks = [b"".join(x + b"\n" for x in lines[i:i + 1500]) for i in range(0, len(lines), 1500)]
    assert len(blocks) > 10
    table = bv.ScoreTable(text=golden[7])
    ctx = bv.Ctx(nh, n_slots=2, score=table, want_class_maps=False, max_batch_bytes=32 << 20, max_lines=4000)
    pending = 0
    first = None
    for k, blk in enumerate(blocks):
        ctx.submit(blk, k)
        pending += 1
        if pending == 2:
            ctx.collect()
            pending -= 1
        if k == len(blocks) // 2:
            first = ctx.scores(reset=True)
    while pending:
        ctx.collect()
        pending -= 1
    second = ctx.scores(reset=True)
    last = ctx.score_words()
    assert not any(x.any() for x in last[:4]) and last[4] == 0
    ctx.close()
    table.close()
    assert first[3] > 0 and second[3] > 0
    got, want = add(first, second), golden_full[0]
    assert want[3] > 1000
    assert same_sums(got, want), sums_diff(got, want)


def score_args(golden, tmp_path):
    (tmp_path / "w.tsv").write_bytes(golden[7])
    return ["--score", str(tmp_path / "w.tsv"), "--scoreOutput", str(tmp_path / "s.tsv")]


def test_golden_cli_keep_samples_and_min_gq(bv, golden, tmp_path):
    """200 kept samples, in rank space, through the masked scan (the slice has no GQ: --minGQ masks nothing)"""
    vcf = golden[0]
    idx = sorted(random.Random(77).sample(range(2504), 200))
    want = golden_files(golden, cols=idx)[1]
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx)
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--keepSamples", lst, "--minGQ", "20"] + score_args(golden, tmp_path))
    assert p.returncode == 0, p.stderr[-400:]
    got = (tmp_path / "s.tsv").read_bytes()
    assert got == want, first_difference(got, want)


def test_golden_cli_regions_and_min_maf(bv, golden, tmp_path):
    """--regions and --minMaf 0.01: the scores over the rows both gates leave"""
    vcf, body, names = golden[:3]
    sets = rg.golden_sets(body)[0]
    mask = [a and b for a, b in zip(rg.select(body, sets), sg.gate(body, len(names), {"minMaf": 0.01})[0])]
    assert 300 < sum(mask) < len(mask) - 1000
    want = golden_files(golden, mask=mask)[1]
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--minMaf", "0.01"] + score_args(golden, tmp_path) + sets.cli_args(tmp_path))
    assert p.returncode == 0, p.stderr[-400:]
    got = (tmp_path / "s.tsv").read_bytes()
    assert got == want, first_difference(got, want)


def test_golden_cli_keep_variants(bv, golden, golden_full, tmp_path):
    """--keepVariants with every other locus: the two tables are independent, the scores are over the rows that stay"""
    body, loci = golden[1], golden[4]
    listed = vl.golden_list(body)
    (tmp_path / "keep.txt").write_bytes(vl.list_text(listed))
    mask = vl.select(body, listed, False)
    want = golden_files(golden, mask=mask)
    assert 0 < want[0][3] < golden_full[0][3]
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--keepVariants", str(tmp_path / "keep.txt")] + score_args(golden, tmp_path))
    assert p.returncode == 0, p.stderr[-400:]
    got = (tmp_path / "s.tsv").read_bytes()
    assert got == want[1], first_difference(got, want[1])


# ---- the CLI (each run under its own time limit)

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("score")
    vcf = vcfgen.gen_vcf(41, 3000, 400, weird=0.02) + vcfgen.gen_vcf(42, 1500, 400, weird=0.02).split(b"\n", 3)[3]
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz", "score": d / "w.tsv"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    text = make_text(vcf, 16, 800, names=[b"C%d" % c for c in range(16)], big=True, frac=0.5)
    paths["score"].write_bytes(text)
    t, want_out, want_rep, out_o, _ = score.expected(orc.run, vcf, text)
    return vcf, paths, d, out_o, (want_out, want_rep)


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        p = cli(args + ["--score", str(paths["score"]), "--scoreOutput", str(d / (tag + ".s")), "--scoreReport", str(d / (tag + ".r"))], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        got = ((d / (tag + ".s")).read_bytes(), (d / (tag + ".r")).read_bytes())
        assert got[1] == want[1], tag
        assert got[0] == want[0], (tag, first_difference(got[0], want[0]))


def test_cli_no_out_scoring_only_pass(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    p = cli(["--in", str(paths["text"]), "--noOut", "--score", str(paths["score"]), "--scoreOutput", str(d / "noout.s")])
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == b""
    assert (d / "noout.s").read_bytes() == want[0]


def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    outs = {}
    for tag, extra in (("plain", []), ("score", ["--score", str(paths["score"]), "--scoreOutput", str(d / "o.s")])):
        tsv, dos, smp, sst, prs = (d / ("%s.%s" % (tag, x)) for x in ("tsv.gz", "arrow", "samples", "stats", "pairs"))
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--compressOutput", "bgzf", "--dosageOutput", str(dos),
                 "--sample", str(smp), "--sampleStats", str(sst), "--relatedness", str(prs), "--plinkOutput", str(d / tag),
                 "--grm", str(d / tag)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        made = [tsv, dos, smp, sst, prs] + [d / (tag + x) for x in (".bed", ".bim", ".fam", ".grm.bin", ".grm.N.bin", ".grm.id")]
        outs[tag] = tuple(hashlib.sha256(f.read_bytes()).hexdigest() for f in made) + (p.stderr,)
    assert outs["plain"] == outs["score"]
    assert (d / "o.s").read_bytes() == want[0]


def test_cli_a_file_without_sample_columns_and_exit_codes(bv, cohort, tmp_path):
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    w = str(cohort[1]["score"])
    p = cli(["--score", w, "--scoreOutput", str(tmp_path / "sites.s"), "--scoreReport", str(tmp_path / "sites.r")], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    head = "\t".join(["sample", "matched", "called", "dosageSum"] + [x for c in range(16) for x in ("C%d_SUM" % c, "C%d_AVG" % c)])
    assert (tmp_path / "sites.s").read_bytes() == head.encode() + b"\n"
    assert (tmp_path / "sites.r").read_bytes().endswith(b"columns\t16\nmatchedRows\t0\n")
    # an unwritable path: one message, nothing on stdout
    bad = tmp_path / "no_such_dir" / "x"
    p = cli(["--score", w, "--scoreOutput", str(bad)], vcf)
    assert p.returncode == 1 and str(bad).encode() in p.stderr and p.stderr.count(b"\n") == 1
    assert p.stdout == b""
