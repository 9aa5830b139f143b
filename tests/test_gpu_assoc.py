"""--pheno / --assoc: the per-row association scan summed on the device (bvcf_assoc.hip.h, bvcf_set_pheno_table, bvcf_assoc)
and the files written from its records.

The expected records and bytes come from the oracle's TSV of the same bytes (assoc.py): class matrices of the rows'
heterozygotes / homozygotes / missingGenos lists, the values by their exact definition, sums in Python integers, the
statistic operation for operation.  Every comparison is integer for integer (the records) or byte for byte (the files):
there is no tolerance."""
import gzip
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import assoc
import bgzf
import grm
import gtmask
import oracle_lib as orc
import pairtable as pt
import regions as rg
import samplecut
import score
import sitegate as sg
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")


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
    """every device path that leaves class maps (as in test_gpu_score.py)"""
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


def rec_tuples(arr):
    """an ASSOC_REC_DTYPE array (rows, K) -> [rows][K] tuples as assoc.records gives them"""
    out = []
    for row in arr:
        out.append([(int(r["n_het"]), int(r["n_hom"]), int(r["n_mis"]), int(r["a_het"]), int(r["a_hom"]), int(r["a_mis"]),
                     (int(r["b_mis_hi"]) << 64) | int(r["b_mis_lo"])) for r in row])
    return out


def ctx_records(bv, vcf, pheno_text, allow="PASS,.", block_lines=None, **kw):
    """the records of a ctx that the file's data lines went through, batch after batch"""
    nh, eol, data = split_file(vcf)
    table = bv.PhenoTable(text=pheno_text, sample_names=[x.encode() for x in pt.sample_names(vcf)])
    ctx = bv.Ctx(nh, allow=allow, eol_chars=eol, pheno=table, **kw)
    out = []
    try:
        lines = data.split(b"\n")[:-1]
        step = block_lines or max(len(lines), 1)
        for i in range(0, len(lines), step):
            ctx.process(b"".join(x + b"\n" for x in lines[i:i + step]))
            out += rec_tuples(ctx.assoc())
        return out
    finally:
        ctx.close()
        table.close()


def run_with_assoc(bv, vcf, pheno_text, tmp_path, cfg=None, **kw):
    """bvcf_run_buffer with --pheno / --assoc -> (rc, TSV body, log, output file, report)"""
    c = dict(cfg or {})
    (tmp_path / "p.tsv").write_bytes(pheno_text)
    c.update(pheno=str(tmp_path / "p.tsv"), assoc=str(tmp_path / "a.tsv"), assocReport=str(tmp_path / "a.report"))
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    return rc, out, log, (tmp_path / "a.tsv").read_bytes(), (tmp_path / "a.report").read_bytes()


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


def records_diff(got, want):
    if len(got) != len(want):
        return "%d rows, want %d" % (len(got), len(want))
    fields = ("N_het", "N_hom", "N_mis", "A_het", "A_hom", "A_mis", "B_mis")
    for r, (a, b) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(a, b)):
            for f, (u, v) in zip(fields, zip(x, y)):
                if u != v:
                    return "row %d phenotype %d %s: got %d want %d" % (r, k, f, u, v)
    return "same"


def check_both(bv, vcf, pheno_text, tmp_path, cfg=None):
    """raw records through a ctx and the files through bvcf_run_buffer, against the oracle's"""
    cfg = cfg or {}
    want, tots, want_out, want_rep, out_o, log_o = assoc.expected(orc.run, vcf, pheno_text, cfg)
    rc, out, log, got_out, got_rep = run_with_assoc(bv, vcf, pheno_text, tmp_path, cfg)
    assert rc == 0, log
    assert out == out_o and log == log_o, "the TSV / log changed with --pheno / --assoc"
    got = ctx_records(bv, vcf, pheno_text, allow=cfg.get("allow", "PASS,."))
    assert got == want, records_diff(got, want)
    assert got_rep == want_rep, (got_rep, want_rep)
    assert got_out == want_out, first_difference(got_out, want_out)
    return want, tots, want_rep


def n_tested(rep):
    return int(rep.split(b"tested\t")[1])


# ---- the kernels

@pytest.mark.parametrize("seed", [s[0] for s in pt.FUZZ])
def test_fuzz(bv, bvcf_path, tmp_path, seed):
    """K = 3 columns of mixed sign and magnitude with some NA; every row and column gets different data, so a transposed C/D
    or a swapped class cannot pass"""
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",",
                                          "emptyField": "NA"}
    vcf = pt.fuzz_vcf(seed)
    names = [b"T%d" % c for c in range(3)] if seed % 2 else None
    want, tots, rep = check_both(bv, vcf, assoc.pheno_for(vcf, 3, seed, names, big=bool(seed & 2)), tmp_path, cfg)
    assert len(want) > 50 and n_tested(rep) > 100


@pytest.mark.parametrize("ns", grm.SAMPLE_EDGES)
def test_sample_edges(bv, two_paths, tmp_path, ns):
    """1 .. 300 samples: a k-step short of, at and past its 64 samples, the pad bits of the last 16 map bytes, five steps (a
    chunk of four and one more) at 300"""
    vcf = grm.edge_vcf(ns)
    want = check_both(bv, vcf, assoc.pheno_for(vcf, 2, 300 + ns, big=True, absent=0.0 if ns < 3 else 0.05), tmp_path)[0]
    assert len(want) > 20


@pytest.mark.parametrize("n_rows", assoc.DENSE_ROWS)
def test_dense_row_tile_edges(bv, monkeypatch, tmp_path, n_rows):
    """1 .. 130 dense rows: a wave's 16 rows and a workgroup's 64 short of, at and past their edges"""
    for k, v in PATHS["streaming"].items():
        monkeypatch.setenv(k, v)
    vcf = assoc.dense_vcf(n_rows)
    want = check_both(bv, vcf, assoc.pheno_for(vcf, 3, 400 + n_rows, big=True), tmp_path)[0]
    assert len(want) == n_rows + 1


def column_case(vcf, k, top, seed):
    """a file with K columns of values up to `top` in size, one of them `top` itself"""
    rng = random.Random(seed)
    rows = []
    for i, nm in enumerate(pt.sample_names(vcf)):
        rows.append((nm.encode(), [top if (i, c) == (0, 0) else rng.randint(-top, top) for c in range(k)]))
    return assoc.file_text(rows)


# K, the largest |Y|, n_cols = K (1 + L1 + L2): below 16; exactly 16 (|Y| = 127 has one limb, its square two); 17 (6 * 10^11 has
# six limbs, its square ten); the maximum -- K = 16 with a value at 10^6 gives L1 = 6, L2 = 11 and 288 columns
COLUMN_CASES = [(1, 11, 3), (5, 11, 15), (4, 127, 16), (1, 6 * 10 ** 11, 17), (16, assoc.MAX_Y, 288)]


@pytest.mark.parametrize("k,top,n_cols", COLUMN_CASES)
def test_column_counts(bv, two_paths, tmp_path, k, top, n_cols):
    vcf = grm.edge_vcf(65)
    text = column_case(vcf, k, top, 500 + k)
    table = bv.PhenoTable(text=text, sample_names=[x.encode() for x in pt.sample_names(vcf)])
    assert table.n_cols == n_cols == k * (1 + assoc.n_limbs(top) + assoc.n_limbs(top * top))
    table.close()
    check_both(bv, vcf, text, tmp_path)


# ---- single cases

def test_both_map_forms(bv, bvcf_path, tmp_path):
    vcf = pt.rare_vcf(300)
    check_both(bv, vcf, assoc.pheno_for(vcf, 4, 610, big=True), tmp_path)


def test_short_list_at_its_limit(bv, bvcf_path, tmp_path):
    """15 entries x 4 samples, missing calls among them"""
    vcf = pt.short_list_limit_vcf()
    check_both(bv, vcf, assoc.pheno_for(vcf, 2, 620, big=True), tmp_path)


def test_missing_samples_missing_rows_and_degenerate_columns(bv, bvcf_path, tmp_path):
    """a sample missing in every row, a row in which every sample is missing, an all-hom row (va = 0), n = 2, haploid
    calls; a column that is all NA, a constant column (vb = 0) and a binary column"""
    vcf = assoc.special_vcf()
    rng = random.Random(630)
    rows = [(nm.encode(), [None, 7 * assoc.ONE, rng.choice([0, assoc.ONE]), rng.randint(-5000, 5000)]) for nm in pt.sample_names(vcf)]
    text = assoc.file_text(rows, [b"allNA", b"constant", b"case", b"bmi"])
    want, tots, rep = check_both(bv, vcf, text, tmp_path)
    ints = [[assoc.ints(r, t) for r, t in zip(row, tots)] for row in want]
    assert all(q[0][0] == 0 for q in ints)                      # all NA: n = 0 everywhere
    assert all(q[1][4] == 0 for q in ints)                      # a constant column: vb = 0
    assert ints[0][3][3] == 0 and ints[0][3][0] > 3             # the all-hom row: va = 0
    assert ints[1][3][0] == 1 and ints[2][3][0] == 2            # one and two called samples
    assert want[1][3][2] == len(rows) - 1                       # everybody but one missing
    assert 0 < n_tested(rep) < 2 * len(want)
    vcf = grm.all_missing_sample_vcf()
    check_both(bv, vcf, assoc.pheno_for(vcf, 2, 631), tmp_path)
    vcf = pt.half_missing_vcf()
    check_both(bv, vcf, assoc.pheno_for(vcf, 2, 632, binary_column=1), tmp_path)


def test_multiallelic_lines(bv, bvcf_path, tmp_path):
    vcf = score.multiallelic_vcf()
    assert len(check_both(bv, vcf, assoc.pheno_for(vcf, 2, 640, big=True), tmp_path)[0]) > 40


def test_b_mis_passes_64_bits(bv, two_paths, tmp_path):
    """300 samples at Y = 10^12, all but one missing in a row: B_mis = 299 * 10^24 needs the high word"""
    vcf = assoc.big_missing_vcf()
    rows = [(nm.encode(), [assoc.MAX_Y, -assoc.MAX_Y]) for nm in pt.sample_names(vcf)]
    want = check_both(bv, vcf, assoc.file_text(rows), tmp_path)[0]
    assert want[0][0][6] == 299 * 10 ** 24 >= 1 << 64 and want[0][1][5] == -299 * 10 ** 12


def test_min_gq_masked_calls_are_missing(bv, bvcf_path, tmp_path):
    vcf = pt.fuzz_vcf(13)  # GT:DP:GQ, CRLF
    masked = gtmask.mask_vcf(vcf, 20, 0)
    text = assoc.pheno_for(vcf, 2, 650, big=True)
    want, tots, want_out, want_rep, _, _ = assoc.expected(orc.run, masked, text)
    assert sum(r[0][2] for r in want) > sum(r[0][2] for r in assoc.expected(orc.run, vcf, text)[0])  # more missing calls
    rc, out, log, got_out, got_rep = run_with_assoc(bv, vcf, text, tmp_path, {"minGQ": 20})
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
    check_both(bv, vcf, assoc.pheno_for(vcf, 5, 660, big=True), tmp_path)
    n, msg = bv.guard_check()
    assert n == 0, "%d buffer(s) written out of bounds, the first: %s" % (n, msg)


# ---- the Ctx

def test_ctx_without_a_table_without_samples_and_with_the_wrong_samples(bv):
    ctx = bv.Ctx(9 + 4)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.assoc_info()
    assert ei.value.rc == bv.E_ARG
    ctx.close()
    table = bv.PhenoTable([[]], [[]])
    ctx = bv.Ctx(9, pheno=table)  # no sample columns: a no-op, and no records
    assert ctx.assoc().shape == (0, 1)
    ctx.close()
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + 4, pheno=table)
    assert ei.value.rc == bv.E_ARG
    table.close()


def test_ctx_above_the_cap(bv):
    """a slot's records past 1 GiB: one message, nothing allocated"""
    table = bv.PhenoTable([[1, 2]] * 16, [[1, 1]] * 16)
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + 2, pheno=table, max_batch_bytes=512 << 20, max_lines=1000)
    assert ei.value.rc == bv.E_TOO_BIG and "1 GiB" in str(ei.value) and "columns" in str(ei.value)
    ctx = bv.Ctx(9 + 2, pheno=table, max_batch_bytes=1 << 20, max_lines=1000)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.reserve_assoc_rows((1 << 30) // (56 * 16) + 1)
    assert ei.value.rc == bv.E_TOO_BIG
    ctx.close()
    table.close()


def test_capacity_grow_and_resubmit(bv, monkeypatch):
    """more rows than the arena holds: the batch comes back BVCF_E_CAPACITY with the need and nothing written; after
    bvcf_reserve_assoc_rows the same block gives the records"""
    for k, v in PATHS["streaming"].items():
        monkeypatch.setenv(k, v)
    vcf = assoc.many_alts_vcf()  # three rows a line at 20 samples: more rows than a line of text is taken to give
    text = assoc.pheno_for(vcf, 2, 670)
    want4 = assoc.expected(orc.run, vcf, text)[0]
    nh, eol, many = split_file(vcf)
    table = bv.PhenoTable(text=text, sample_names=[x.encode() for x in pt.sample_names(vcf)])
    ctx = bv.Ctx(nh, eol_chars=eol, pheno=table, max_batch_bytes=64 << 10, max_lines=4000, max_alleles=8000)  # (an arena of 512 rows)
    assert len(want4) > 512 and len(many) < 64 << 10
    ctx.submit(many)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.collect()
    assert ei.value.rc == bv.E_CAPACITY
    info = ctx.assoc_info()
    assert info.need_rows == len(want4) and info.n_rows == 0
    ctx.reserve_assoc_rows(info.need_rows)
    ctx.process(many)
    got = rec_tuples(ctx.assoc())
    ctx.close()
    table.close()
    assert got == want4, records_diff(got, want4)


# ---- the 1KG slice: 2 504 samples, 40 k-steps

@pytest.fixture(scope="module")
def golden(golden_1kg):
    """the slice's TSV body and class matrices through the oracle, once, with three phenotypes"""
    vcf = golden_1kg[0]
    rc, body, _, _ = orc.run(vcf)
    assert rc == 0
    names = pt.sample_names(vcf)
    H, O, M = pt.matrices(body, names)
    for x in (H, O, M):
        x.setflags(write=False)
    cols = [b"height", b"case", b"big"]
    rng = random.Random(700)
    rows = []
    for nm in names:
        if rng.random() < 0.03:
            continue
        rows.append((nm.encode(), [None if rng.random() < 0.05 else rng.randint(-40 * assoc.ONE, 40 * assoc.ONE), rng.choice([0, assoc.ONE]),
                                   rng.randint(-assoc.MAX_Y, assoc.MAX_Y)]))
    return vcf, body, names, (H, O, M), assoc.loci_columns(body), cols, assoc.file_text(rows, cols)


def golden_files(golden, mask=None, cols=None):
    """the records and the output file of the slice's rows that stay (mask) over the samples that stay (cols; a row no kept
    sample carries is no row)"""
    vcf, body, names, (H, O, M), loci, colnames, text = golden
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
    return assoc.expected_m(H, O, M, loci, names, text)


def cli(args, stdin_bytes=None, timeout=300, env=None):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout, env=env)


def test_golden_many_batches_with_a_grow(bv, golden, monkeypatch):
    """the slice in batches of 1 500 lines, two in flight, maps made on the device only; the ctx reserves 1 000 lines, so the
    first batch comes back BVCF_E_CAPACITY, the reservations grow -- the scan's row lists with them -- and the batches in
    flight are submitted again"""
    monkeypatch.setenv("BVCF_PATH", "2")
    vcf = golden[0]
    want = golden_files(golden)[0]
    nh, eol, data = split_file(vcf)
    lines = data.split(b"\n")[:-1]
    blocks = [b"".join(x + b"\n" for x in lines[i:i + 1500]) for i in range(0, len(lines), 1500)]
    assert len(blocks) > 10
    table = bv.PhenoTable(text=golden[6], sample_names=[x.encode() for x in golden[2]])
    ctx = bv.Ctx(nh, n_slots=2, pheno=table, want_class_maps=False, max_batch_bytes=32 << 20, max_lines=1000)
    got, grown = [], 0
    queue = list(range(len(blocks)))
    in_flight = []
    while queue or in_flight:
        while queue and len(in_flight) < 2:
            k = queue.pop(0)
            ctx.submit(blocks[k], k)
            in_flight.append(k)
        try:
            ctx.collect()
        except bv.BvcfError as e:
            assert e.rc == bv.E_CAPACITY
            need = ctx.assoc_info().need_rows
            for _ in in_flight[1:]:
                try:
                    ctx.collect()
                except bv.BvcfError:
                    pass
            ctx.reserve(4000, 8000, 8 << 20)
            ctx.reserve_assoc_rows(max(need, 1))
            grown += 1
            assert grown < 4
            queue = in_flight + queue
            in_flight = []
            continue
        in_flight.pop(0)
        got += rec_tuples(ctx.assoc())
    ctx.close()
    table.close()
    assert len(want) > 10000 and grown >= 1
    assert got == want, records_diff(got, want)


def assoc_args(golden, tmp_path):
    (tmp_path / "p.tsv").write_bytes(golden[6])
    return ["--pheno", str(tmp_path / "p.tsv"), "--assoc", str(tmp_path / "a.tsv")]


def test_golden_cli_keep_samples_and_min_gq(bv, golden, tmp_path):
    """200 kept samples, in rank space, through the masked scan (the slice has no GQ: --minGQ masks nothing); the file's other
    names are no kept sample and are ignored"""
    vcf = golden[0]
    idx = sorted(random.Random(77).sample(range(2504), 200))
    want = golden_files(golden, cols=idx)[2]
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx)
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--keepSamples", lst, "--minGQ", "20"] + assoc_args(golden, tmp_path))
    assert p.returncode == 0, p.stderr[-400:]
    got = (tmp_path / "a.tsv").read_bytes()
    assert got == want, first_difference(got, want)


def test_golden_cli_regions_and_min_maf(bv, golden, tmp_path):
    """--regions and --minMaf 0.01: the scan over the rows both gates leave"""
    vcf, body, names = golden[:3]
    sets = rg.golden_sets(body)[0]
    mask = [a and b for a, b in zip(rg.select(body, sets), sg.gate(body, len(names), {"minMaf": 0.01})[0])]
    assert 300 < sum(mask) < len(mask) - 1000
    want = golden_files(golden, mask=mask)
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--minMaf", "0.01", "--assocReport", str(tmp_path / "a.rep")] + assoc_args(golden, tmp_path) +
            sets.cli_args(tmp_path))
    assert p.returncode == 0, p.stderr[-400:]
    got = (tmp_path / "a.tsv").read_bytes()
    assert got == want[2], first_difference(got, want[2])
    assert (tmp_path / "a.rep").read_bytes() == want[3]


# ---- the CLI (each run under its own time limit)

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc")
    vcf = vcfgen.gen_vcf(41, 3000, 400, weird=0.02) + vcfgen.gen_vcf(42, 1500, 400, weird=0.02).split(b"\n", 3)[3]
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz", "pheno": d / "p.tsv"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    text = assoc.pheno_for(vcf, 4, 800, names=[b"P%d" % c for c in range(4)], big=True, binary_column=1)
    paths["pheno"].write_bytes(text)
    recs, tots, want_out, want_rep, out_o, _ = assoc.expected(orc.run, vcf, text)
    return vcf, paths, d, out_o, (want_out, want_rep)


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        p = cli(args + ["--pheno", str(paths["pheno"]), "--assoc", str(d / (tag + ".a")), "--assocReport", str(d / (tag + ".r"))], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        got = ((d / (tag + ".a")).read_bytes(), (d / (tag + ".r")).read_bytes())
        assert got[1] == want[1], tag
        assert got[0] == want[0], (tag, first_difference(got[0], want[0]))


def test_cli_no_out_scan_only_pass(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    p = cli(["--in", str(paths["text"]), "--noOut", "--pheno", str(paths["pheno"]), "--assoc", str(d / "noout.a")])
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == b""
    assert (d / "noout.a").read_bytes() == want[0]


def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    outs = {}
    for tag, extra in (("plain", []), ("assoc", ["--pheno", str(paths["pheno"]), "--assoc", str(d / "o.a")])):
        tsv, dos, smp, sst, prs = (d / ("%s.%s" % (tag, x)) for x in ("tsv.gz", "arrow", "samples", "stats", "pairs"))
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--compressOutput", "bgzf", "--dosageOutput", str(dos),
                 "--sample", str(smp), "--sampleStats", str(sst), "--relatedness", str(prs), "--plinkOutput", str(d / tag),
                 "--grm", str(d / tag)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        made = [tsv, dos, smp, sst, prs] + [d / (tag + x) for x in (".bed", ".bim", ".fam", ".grm.bin", ".grm.N.bin", ".grm.id")]
        outs[tag] = tuple(hashlib.sha256(f.read_bytes()).hexdigest() for f in made) + (p.stderr,)
    assert outs["plain"] == outs["assoc"]
    assert (d / "o.a").read_bytes() == want[0]


def test_cli_a_file_without_sample_columns_and_exit_codes(bv, cohort, tmp_path):
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    f = str(cohort[1]["pheno"])
    p = cli(["--pheno", f, "--assoc", str(tmp_path / "sites.a"), "--assocReport", str(tmp_path / "sites.r")], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    assert (tmp_path / "sites.a").read_bytes() == (assoc.HEADER + "\n").encode()
    assert (tmp_path / "sites.r").read_bytes() == b"columns\t4\nsamples\t0\nrows\t0\ntested\t0\n"
    # an unwritable path: one message, nothing on stdout
    bad = tmp_path / "no_such_dir" / "x"
    p = cli(["--pheno", f, "--assoc", str(bad)], vcf)
    assert p.returncode == 1 and str(bad).encode() in p.stderr and p.stderr.count(b"\n") == 1
    assert p.stdout == b""
    # a bad phenotype file and an unreadable one: one message that names the line, exit code 1, no row written (the file is
    # matched against the sample names, so the TSV's header line is out by then), the output left empty
    cohort_vcf = cohort[0]
    (tmp_path / "bad.tsv").write_bytes(b"#sample\ta\nS1\t1\nS2\tx\n")
    p = cli(["--pheno", str(tmp_path / "bad.tsv"), "--assoc", str(tmp_path / "bad.a")], cohort_vcf)
    assert p.returncode == 1 and b"line 3:" in p.stderr and p.stderr.count(b"\n") == 1 and p.stdout.count(b"\n") <= 1
    assert (tmp_path / "bad.a").read_bytes() == b""
    p = cli(["--pheno", str(tmp_path / "none.tsv"), "--assoc", str(tmp_path / "none.a")], cohort_vcf)
    assert p.returncode == 1 and b"none.tsv" in p.stderr and p.stderr.count(b"\n") == 1 and p.stdout.count(b"\n") <= 1
    # flags without their partner: exit code 2
    for args in (["--pheno", f], ["--assoc", "x"], ["--assocReport", "x"], ["--pheno"]):
        p = cli(args, vcf)
        assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1
