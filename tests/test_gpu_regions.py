"""Row selection by genomic interval on the device (bvcf_regions.hip.h, bvcf_set_region_table): whole runs with --regions /
--regionsFile / --excludeRegions / --excludeRegionsFile against the oracle's run of the same bytes with the unselected rows
taken out (regions.select) -- the TSV, the log, the records and dosage rows, the report, and every other output as the
reference of its own module over the rows that stay -- and against a second run of the same build with --keepVariants L,
L the loci the Python reference keeps: equal loci have equal spans, so the two runs agree on every output.
tests/test_regions_cpu.py checks the inputs used here with the oracle alone."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import bgzf
import ldpairs as lp
import mendel as md
import oracle_lib as orc
import pairtable as pt
import plinkbed as pb
import regions as rg
import samplecut
import sitegate as sg
import variantlist as vl
from test_gpu_sample_stats import table_from_tsv
from test_gpu_site_gate import blocks_of, first_diff, oracle_dosage_kept, split_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")

CHAINS = {"census": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0"},
          "streaming": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "0"},
          "streaming-general": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "1"}}


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


@pytest.fixture(params=list(CHAINS))
def chain(request, monkeypatch):
    for k, v in CHAINS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


_ORACLE = {}


def oracle_side(vcf, cfg=None):
    cfg = cfg or {}
    key = (hashlib.sha256(vcf).digest(), tuple(sorted(cfg.items())))
    if key not in _ORACLE:
        rc, out, log, _ = orc.run(vcf, cfg)
        assert rc == 0
        _ORACLE[key] = (out, log)
    return _ORACLE[key]


_WANT = {}


def expected(bv, vcf, sets, cfg=None, gate=None, variants=None):
    """what a run of `vcf` with the regions must produce, from the oracle's run of the same bytes: computed once, shared by
    the chains.  variants = (loci, exclude): a list that acts behind the regions; gate: site-gate criteria behind both"""
    cfg = cfg or {}
    key = (hashlib.sha256(vcf).digest(), sets.key(), tuple(sorted(cfg.items())), tuple(sorted((gate or {}).items())),
           None if variants is None else (hashlib.sha256(b"\n".join(variants[0])).digest(), bool(variants[1])))
    if key not in _WANT:
        out, log = oracle_side(vcf, cfg)
        names = pt.sample_names(vcf)
        mask = rg.select(out, sets, bool(names))
        body = sg.kept_body(out, mask)
        w = {"log": log, "names": names, "counts": vl.counts(mask, bool(names)), "loci": rg.kept_loci(out, mask)}
        w["report"] = sets.report(w["counts"])
        if variants is not None:  # the regions go first: the list examines the rows that are left, its report counts those
            vmask = vl.select(body, variants[0], variants[1], bool(names))
            w["variant_report"] = vl.report_text(len(set(variants[0])), vl.counts(vmask, bool(names)))
            body = sg.kept_body(body, vmask)
            it = iter(vmask)
            mask = [m and next(it) for m in mask]
        if gate:
            gmask, gcounts, greport = sg.gate(body, len(names), gate, cfg)
            body = sg.kept_body(body, gmask)
            it = iter(gmask)
            mask = [m and next(it) for m in mask]
            w["site_report"] = greport
        w["mask"], w["body"] = list(mask), body
        if names:
            w["stats"] = table_from_tsv(bv, body, names, cfg)
            w["pairs"] = pt.file_text(pt.tables(*pt.matrices(body, names, cfg)), names, cfg.get("emptyField", "!"))
        _WANT[key] = w
    return _WANT[key]


def write_list(tmp_path, loci, tag="list"):
    p = tmp_path / ("%s.txt" % tag)
    p.write_bytes(vl.list_text(loci))
    return str(p)


def check_run(bv, vcf, sets, tmp_path, cfg=None, expect_of=None, gate=None, variants=None, tag="r", twin=True, **kw):
    """bvcf_run_buffer of the original bytes with the regions, the reports and the two tables against the references; then
    -- twin -- the run with --keepVariants L in the regions' place, which must write the same TSV and tables.  expect_of:
    the bytes the oracle runs (the masked or cut file of a composed case)"""
    cfg = dict(cfg or {})
    base = {k: v for k, v in cfg.items() if k not in ("minGQ", "minDP", "keepSamples", "excludeSamples")}
    w = expected(bv, vcf if expect_of is None else expect_of, sets, base, gate, variants)
    files = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("sampleStats", "relatedness", "regionFilterReport")}
    if gate:
        files["siteFilterReport"] = str(tmp_path / ("%s.site" % tag))
    if variants is not None:
        files["variantFilterReport"] = str(tmp_path / ("%s.vrep" % tag))
    run_cfg = dict(cfg, **(gate or {}), **files, **sets.cfg(tmp_path, tag))
    if variants is not None:
        run_cfg["excludeVariants" if variants[1] else "keepVariants"] = write_list(tmp_path, variants[0], tag + ".v")
    rc, out, log, _ = bv.run_buffer(vcf, run_cfg, **kw)
    assert rc == 0, log
    assert out == w["body"], first_diff(out, w["body"])
    assert log == w["log"]
    got = {k: open(p, "rb").read() for k, p in files.items()}
    assert got["regionFilterReport"] == w["report"], (got["regionFilterReport"], w["report"])
    if w["names"]:
        assert got["sampleStats"] == w["stats"], first_diff(got["sampleStats"], w["stats"])
        assert got["relatedness"] == w["pairs"], first_diff(got["relatedness"], w["pairs"])
    if gate:
        assert got["siteFilterReport"] == w["site_report"], (got["siteFilterReport"], w["site_report"])
    if variants is not None:
        assert got["variantFilterReport"] == w["variant_report"], (got["variantFilterReport"], w["variant_report"])
    if twin and variants is None and w["names"]:
        tfiles = {k: str(tmp_path / ("%s.twin.%s" % (tag, k))) for k in ("sampleStats", "relatedness")}
        if gate:
            tfiles["siteFilterReport"] = str(tmp_path / ("%s.twin.site" % tag))
        rc, tout, tlog, _ = bv.run_buffer(vcf, dict(cfg, **(gate or {}), **tfiles, keepVariants=write_list(tmp_path, w["loci"], tag + ".twin")), **kw)
        assert rc == 0 and tout == out and tlog == log
        for k, p in tfiles.items():
            assert open(p, "rb").read() == got[k], k
    return w


def check_records(bv, vcf, sets, cfg=None, expect_of=None, **ctx_kw):
    """the file's blocks through a ctx with the table: every examined record's ac, an .. n_miss, pad[0] and pad[1] against
    the oracle's rows and the mask, the batches' counts, and the dosage rows of the rows that stay against the oracle's.
    -> the (flags, pos) of the examined records"""
    cfg = cfg or {}
    ref = vcf if expect_of is None else expect_of
    w = expected(bv, ref, sets, cfg)
    out, _ = oracle_side(ref, cfg)
    S = len(w["names"])
    rows = [sg.row_counts(r.split(b"\t"), cfg) for r in vl.rows_of(out)]
    if "dosage" not in w:
        w["dosage"] = oracle_dosage_kept(ref, cfg, w["mask"])[1]
    nh, eol, data = split_file(vcf)
    table = sets.table(bv)
    ctx = bv.Ctx(nh, allow=cfg.get("allow", "PASS,."), eol_chars=eol, want_dosage=True, regions=table, **ctx_kw)
    counts = [0, 0, 0]
    examined, dosage, flags = [], [], []
    for blk in blocks_of(data):
        b = ctx.process(blk)
        counts = [x + y for x, y in zip(counts, b.region_counts)]
        # the list's and the site gate's view: the kept rows, no more
        assert b.variant_counts == [b.region_counts[1], b.region_counts[1], 0]
        assert b.gate_counts[0] == b.gate_counts[1] == b.region_counts[1]
        kept_slots = []
        for i in range(b.n_lines):
            if int(b.lines[i]["status"]) != bv.LINE_OK:
                continue
            for k in b.record_slots(i):
                A = b.alleles[k]
                p0, p1 = int(A["pad"][0]), int(A["pad"][1])
                assert p0 == 0 and p1 in (0, 2)
                if int(A["ac"]) == 0 and p1 == 0:
                    continue  # a row no sample carries: not examined
                assert (int(A["ac"]) == 0) == (p1 == 2), "a row the regions took out has ac == 0 and pad[1] == 2"
                examined.append((int(A["ac"]), int(A["an"]), int(A["n_het"]), int(A["n_hom"]), int(A["n_miss"])))
                flags.append((int(A["flags"]), int(A["pos"])))
                if p1 == 0:
                    kept_slots.append(k)
        dosage.append(np.array(b.dosage[np.array(kept_slots, dtype=np.int64), :S], dtype=np.int8).reshape(len(kept_slots), S))
    ctx.close()
    assert counts == w["counts"], (counts, w["counts"])
    assert len(examined) == len(rows) == len(w["mask"])
    for got, c, keep in zip(examined, rows, w["mask"]):
        assert got == ((c[0] if keep else 0),) + c[1:], (got, c, keep)  # an .. n_miss stay as they were
    dosage = np.concatenate(dosage) if dosage else np.zeros((0, S), dtype=np.int8)
    assert dosage.shape == w["dosage"].shape
    bad = np.argwhere(dosage != w["dosage"])
    assert not len(bad), "dosage: %d cells differ, first at kept row %d sample %d" % (len(bad), bad[0][0], bad[0][1])
    return flags


# ---- spans at the edges, every kind of row

EDGE_SETS = {"keep": rg.Sets(regions=rg.EDGE_KEEP), "exclude": rg.Sets(exclude=rg.EDGE_KEEP),
             "both": rg.Sets(regions=rg.EDGE_KEEP, exclude=rg.EDGE_EXCLUDE),
             "bed": rg.Sets(regions_bed=rg.bed_text(rg.parse_specs(b"7:1000-2000,7:3000")), regions=b"7:5000-")}


@pytest.mark.parametrize("which", list(EDGE_SETS))
@pytest.mark.parametrize("ns", [1, 5])
def test_spans_at_the_edges(bv, chain, tmp_path, ns, which):
    """pos at beg - 1, beg, end, end + 1; deletions that touch with their first or last base, fall one base short, cover an
    interval; multiallelic lines and MNPs that the edge cuts; insertions at the edge; POS texts that are no positions;
    rows with the POS bytes as their only position beside rows whose record holds it"""
    vcf, sets = rg.edges_vcf(ns), EDGE_SETS[which]
    w = check_run(bv, vcf, sets, tmp_path)
    assert 0 < w["counts"][1] < w["counts"][0]
    if which == "bed":
        assert w["body"] == expected(bv, vcf, EDGE_SETS["keep"])["body"]  # (the same set, given as a BED and a SPEC)
    flags = check_records(bv, vcf, sets)
    text = [(f, p) for f, p in flags if f & bv.ALLELE_POS_TEXT]
    # plain SNP lines and simple insertions leave pos = 0 in the record -- the POS bytes are the only source --, deletions,
    # MNPs and the insertions k_head places carry it
    assert len(text) > 20 and all(p == 0 for _, p in text)
    assert len(flags) - len(text) > 10 and all(p != 0 for f, p in flags if not f & bv.ALLELE_POS_TEXT)


def test_keep_and_exclude_on_one_deletion(bv, tmp_path):
    """-10 at 2000 overlaps the keep set with its first base and the exclude set with its first two: it is dropped"""
    vcf = (rg.vcfgen.header(2) + rg._line("7", 1999, "ACGTACGTACG", "A", 2) + rg._line("7", 1000, "A", "T", 2)).encode()
    w = check_run(bv, vcf, EDGE_SETS["both"], tmp_path)
    assert w["mask"] == [False, True]
    w = check_run(bv, vcf, EDGE_SETS["keep"], tmp_path, tag="k")
    assert w["mask"] == [True, True]


# ---- chromosome names

@pytest.mark.parametrize("which", ["keep", "exclude", "both"])
def test_chromosome_names(bv, chain, tmp_path, which):
    """`1` against `chr1`, `chr1` against `chr10`, `chrM`, a long contig, names with ':'; chromosomes with keep intervals
    only, with exclude intervals only and with neither"""
    sets = {"keep": rg.Sets(regions=rg.NAMES_KEEP), "exclude": rg.Sets(exclude=rg.NAMES_EXCLUDE),
            "both": rg.Sets(regions=rg.NAMES_KEEP, exclude=rg.NAMES_EXCLUDE)}[which]
    vcf = rg.names_vcf(3)
    w = check_run(bv, vcf, sets, tmp_path)
    assert 0 < w["counts"][1] < w["counts"][0]
    check_records(bv, vcf, sets)


def test_probe_chain_that_wraps(bv, chain, tmp_path):
    """four names with home slot 15 of 16 (the chain 15, 0, 1, 2); the file also holds names that walk the chain and are
    not in it"""
    listed, every = rg.wrap_case(bv)
    vcf, spec = rg.ctg_vcf(every), b",".join(rg.ctg(i) for i in listed)
    for sets in (rg.Sets(regions=spec), rg.Sets(exclude=spec)):
        w = check_run(bv, vcf, sets, tmp_path, tag="x%d" % (sets.keep is None))
        assert w["mask"] == [(i in listed) == (sets.keep is not None) for i in every]
        check_records(bv, vcf, sets)


def test_collision_pair(bv, chain, tmp_path):
    """the table holds A; the file holds B != A with A's tag and home slot: B goes under keep and stays under exclude"""
    listed, in_file = rg.collision_case(bv)
    a, b = rg.collision_pair(bv)
    vcf, spec = rg.ctg_vcf(in_file), b",".join(rg.ctg(i) for i in listed)
    for sets in (rg.Sets(regions=spec), rg.Sets(exclude=spec)):
        w = check_run(bv, vcf, sets, tmp_path, tag="x%d" % (sets.keep is None))
        assert w["mask"][in_file.index(b)] == (sets.keep is None)
        assert w["mask"] == [(i in listed) == (sets.keep is not None) for i in in_file]
        check_records(bv, vcf, sets)


# ---- interval counts

def test_interval_counts(bv, chain, tmp_path):
    """0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16 and 17 intervals on a chromosome, rows before the first, at and beside every edge,
    between each pair and after the last"""
    vcf, bed = rg.counts_vcf_and_bed()
    for sets in (rg.Sets(regions_bed=bed), rg.Sets(exclude_bed=bed)):
        w = check_run(bv, vcf, sets, tmp_path, tag="x%d" % (sets.keep is None))
        assert 0 < w["counts"][1] < w["counts"][0]
        assert w["report"].startswith(b"keepIntervals\t%d\nexcludeIntervals\t%d\n" % ((87, 0) if sets.keep is not None else (0, 87)))
        check_records(bv, vcf, sets)


def test_empty_sets(bv, chain, tmp_path):
    vcf = vl.rows_vcf(65)
    for bed in (b"", b"# nothing\nchr1\t5\t5\n"):
        w = check_run(bv, vcf, rg.Sets(regions_bed=bed), tmp_path, tag="keep")
        assert w["body"] == b"" and w["counts"] == [65, 0, 65] and w["report"].startswith(b"keepIntervals\t0\nexcludeIntervals\t0\n")
        w = check_run(bv, vcf, rg.Sets(exclude_bed=bed), tmp_path, tag="excl")
        assert w["body"] == oracle_side(vcf)[0] and w["counts"] == [65, 65, 0]
    check_records(bv, vcf, rg.Sets(regions_bed=b""))
    check_records(bv, vcf, rg.Sets(exclude_bed=b""))
    # an empty keep set beside an exclude set that is not empty, and the reverse
    w = check_run(bv, vcf, rg.Sets(regions_bed=b"", exclude=b"chr1"), tmp_path, tag="ke")
    assert w["body"] == b""
    w = check_run(bv, vcf, rg.Sets(regions=b"chr1", exclude_bed=b""), tmp_path, tag="ek")
    assert w["counts"] == [65, 22, 43]


# ---- run shapes

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts_at_the_wave_edges(bv, chain, tmp_path, n):
    vcf, sets = vl.rows_vcf(n), rg.rows_sets(n)
    w = check_run(bv, vcf, sets, tmp_path)
    assert w["counts"][0] == n and (n == 1 or 0 < w["counts"][1] < n)
    check_records(bv, vcf, sets)
    flipped = rg.Sets(exclude=sets.regions)
    w2 = check_run(bv, vcf, flipped, tmp_path, tag="x")
    assert w2["mask"] == [not m for m in w["mask"]]
    check_records(bv, vcf, flipped)


@pytest.fixture(scope="module")
def stride(bv):
    ctx = bv.Ctx(9 + 1)
    n = ctx.region_gate_stride()
    ctx.close()
    assert n and n % 256 == 0
    return n


def test_one_row_more_than_a_grid_step(bv, chain, tmp_path, stride):
    """one batch whose rows outnumber k_region_gate's threads by one: the last row is the second step of thread 0"""
    n = stride + 1
    vcf = vl.rows_vcf(n, 1)
    assert len(vcf) < 48 << 20
    last = 1000 + n - 1  # (the last row, the one of the second step, is named by an interval of its own)
    sets = rg.Sets(regions=b"chr1:1000-%d,chr2:%d-%d,chr%d:%d" % (1000 + n // 2, 1000 + n // 4, 1000 + n // 3, 1 + (n - 1) % 3, last))
    pos = np.arange(n) + 1000
    ch = np.arange(n) % 3
    keep = ((ch == 0) & (pos <= 1000 + n // 2)) | ((ch == 1) & (pos >= 1000 + n // 4) & (pos <= 1000 + n // 3)) | (pos == last)
    w = expected(bv, vcf, sets)
    assert w["mask"] == [bool(x) for x in keep] and keep[-1] and not keep[-2]
    rc, out, log, _ = bv.run_buffer(vcf, sets.cfg(tmp_path))
    assert rc == 0, log
    assert out == w["body"], first_diff(out, w["body"])
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, eol_chars=eol, regions=sets.table(bv), max_lines=n + 64, max_alleles=2 * n + 1024, cmap_bytes=96 * n)
    b = ctx.process(data)
    got_counts = b.region_counts  # (counted from the slot's own arrays: while the ctx lives)
    ctx.close()
    assert b.n_lines == n and (b.lines["status"] == bv.LINE_OK).all() and (b.lines["n_rec"] == 1).all()
    A = b.alleles[:n]
    assert np.array_equal(A["ac"] != 0, keep) and np.array_equal(A["pad"][:, 1] == 2, ~keep) and not A["pad"][:, 0].any()
    assert got_counts == [n, int(keep.sum()), int((~keep).sum())]


# ---- order and composition

def test_regions_then_list_then_site_gate(bv, chain, tmp_path):
    """the list examines the rows the regions leave, the gate the rows the list leaves: all three reports"""
    vcf = sg.case_input("sweep")
    body = oracle_side(vcf)[0]
    sets = rg.half_sets(body)
    left = sg.kept_body(body, rg.select(body, sets))
    lst = vl.every_other(vl.loci_of(left)) + vl.every_other(vl.loci_of(body), 1)[:40]  # (some entries name rows the regions took out)
    for exclude in (False, True):
        w = check_run(bv, vcf, sets, tmp_path, gate=sg.SWEEP, variants=(lst, exclude), tag="x%d" % exclude)
        n_left = w["counts"][1]
        assert w["variant_report"].split(b"\n")[1] == b"examined\t%d" % n_left and 0 < n_left < w["counts"][0]
        n_listed = int(w["variant_report"].split(b"\n")[2].split(b"\t")[1])
        assert w["site_report"].startswith(b"examined\t%d\n" % n_listed) and 0 < w["body"].count(b"\n") < n_listed < n_left
    check_run(bv, vcf, sets, tmp_path, gate=sg.SWEEP, tag="g")  # the gate alone behind the regions, and its twin


def test_composed_with_min_gq(bv, tmp_path):
    vcf, masked = sg.case_input("fuzz13"), sg.case_input("masked13")
    sets = rg.half_sets(oracle_side(masked)[0])
    check_run(bv, vcf, sets, tmp_path, {"minGQ": sg.MASK_GQ}, expect_of=masked)
    check_records(bv, vcf, sets, expect_of=masked, min_gq=sg.MASK_GQ)


def test_composed_with_keep_samples(bv, tmp_path):
    vcf, cut = sg.case_input("rare300"), sg.case_input("cut300")
    half = rg.half_sets(oracle_side(cut)[0])
    sets = rg.Sets(exclude=half.regions)
    names = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], sg.CUT_KEEP)
    check_run(bv, vcf, sets, tmp_path, {"keepSamples": names}, expect_of=cut)
    check_records(bv, vcf, sets, expect_of=cut, sample_keep=sg.CUT_KEEP)


def twin_files(bv, vcf, sets, tmp_path, extra, outputs):
    """a run with the regions and a run with --keepVariants L, both with the side outputs of `extra` (name -> path suffix)
    -> the expected, and the region run's files, which the list run's equal byte for byte"""
    w = expected(bv, vcf, sets)
    got = {}
    for tag, sel in (("r", sets.cfg(tmp_path)), ("l", {"keepVariants": write_list(tmp_path, w["loci"])})):
        cfg = dict(sel, **{k: (str(tmp_path / (tag + v)) if isinstance(v, str) and v.startswith(".") else v) for k, v in extra.items()})
        rc, out, log, _ = bv.run_buffer(vcf, cfg)
        assert rc == 0 and out == w["body"] and log == w["log"], log
        got[tag] = {o: (tmp_path / (tag + o)).read_bytes() for o in outputs}
    assert got["r"] == got["l"]
    return w, got["r"]


def test_plink_fileset_and_dosage_hold_the_kept_rows(bv, chain, tmp_path):
    vcf, sets = rg.edges_vcf(5), EDGE_SETS["both"]
    w, got = twin_files(bv, vcf, sets, tmp_path, {"plinkOutput": ".q", "dosageOutput": ".dosage"}, [".q.bed", ".q.bim", ".q.fam", ".dosage"])
    files = pb.read_files(tmp_path / "r.q")
    assert pb.diff(files, pb.expected_from_body(w["body"], w["names"])) == ""
    assert [ln.split(b"\t")[1] for ln in files["bim"].split(b"\n") if ln] == vl.loci_of(w["body"])
    # (the dosage file is Arrow IPC: held against the list run's byte for byte above; check_records holds the rows against the oracle's)
    assert got[".dosage"].startswith(b"ARROW1") and len(vl.rows_of(w["body"])) > 0


def test_mendel_counts_the_kept_rows(bv, chain, tmp_path):
    vcf, fam = vl.pedigree_case()
    sets = rg.half_sets(oracle_side(vcf)[0])
    (tmp_path / "fam").write_bytes(fam)
    w, got = twin_files(bv, vcf, sets, tmp_path, {"fam": str(tmp_path / "fam"), "mendel": ".mendel", "mendelErrors": ".errors"},
                        [".mendel", ".errors"])
    want = md.expected_from_body(w["body"], w["names"], fam)
    assert int(want["counts"].sum()) > 0
    assert got[".mendel"] == want["mendel"] and got[".errors"] == want["errors"]


def test_ld_window_is_over_the_thinned_rows(bv, chain, tmp_path):
    vcf, window = vl.round_trip_input()
    body = oracle_side(vcf)[0]
    lo, hi = rg.golden_span(body)
    step = max((hi - lo) // 60, 2)
    chroms = sorted({r.split(b"\t")[rg.CHROM] for r in vl.rows_of(body)})
    sets = rg.Sets(exclude_bed=rg.bed_text([(c, lo + j * step, lo + j * step + step // 2) for c in chroms for j in range(61)]))
    w, got = twin_files(bv, vcf, sets, tmp_path, {"ld": ".ld", "ldPrune": ".p", "ldWindow": 7}, [".ld", ".p.prune.in", ".p.prune.out"])
    want = lp.expected_from_body(w["body"], w["names"], 7, 200000)
    full = lp.expected_from_body(body, w["names"], 7, 200000)
    assert len(want["events"]) > 10 and want["table"] != full["table"] and 0 < w["counts"][1] < w["counts"][0]
    assert got[".ld"] == want["table"] and got[".p.prune.in"] == want["prune_in"] and got[".p.prune.out"] == want["prune_out"]


def test_set_region_table_on_a_ctx(bv):
    line = b"chr1\t100\t.\tA\tC\t50\tPASS\t.\tGT\t0|1\n"
    ctx = bv.Ctx(9, regions=bv.RegionTable(keep=b"chr2"))  # no sample columns: a no-op
    b = ctx.process(b"chr1\t100\t.\tA\tC\t50\tPASS\t.\n")
    assert b.region_counts == [0, 0, 0]
    ctx.close()
    ctx = bv.Ctx(9 + 1)  # without a table: every row is examined and kept, nothing is marked
    b = ctx.process(line)
    assert b.region_counts == [1, 1, 0] and not b.alleles["pad"].any()
    ctx.close()
    ctx = bv.Ctx(9 + 1, regions=bv.RegionTable())  # a table without a set: off
    b = ctx.process(line)
    assert b.region_counts == [1, 1, 0] and not b.alleles["pad"].any()
    ctx.close()
    ctx = bv.Ctx(9 + 1, regions=bv.RegionTable(keep=b"chr2"))
    b = ctx.process(line)
    assert b.region_counts == [1, 0, 1] and int(b.alleles[0]["pad"][1]) == 2 and int(b.alleles[0]["ac"]) == 0
    ctx.close()
    # a struct that was never built
    ctx = bv.Ctx(9 + 1)
    raw = bv.RegionTableStruct()
    bv.lib.bvcf_set_region_table.argtypes = [bv.C.c_void_p, bv.C.c_void_p]
    assert bv.lib.bvcf_set_region_table(ctx.h, bv.C.byref(raw)) == bv.E_ARG
    # with a batch in flight
    t = bv.RegionTable(exclude=b"chr1")
    ctx.submit(line)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.set_region_table(t)
    assert ei.value.rc == bv.E_BUSY
    b = ctx.collect()
    assert b.region_counts == [1, 1, 0]
    ctx.set_region_table(t)
    assert ctx.process(line).region_counts == [1, 0, 1]
    ctx.close()


# ---- the CLI (each run under its own time limit)

def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


def test_cli_sites_only_comes_out_unchanged(bv, tmp_path):
    vcf = rg.sites_vcf(300)
    plain = cli([], vcf)
    assert plain.stdout.count(b"\n") == 1 + 300 + 100  # (the header line, 200 SNP rows and 100 lines of two rows)
    for args in (["--regions", "chr1:1-1000,2"], ["--excludeRegions", "1,2,3"], ["--regions", "nowhere"]):
        rep = tmp_path / "sites.report"
        p = cli(args + ["--regionFilterReport", str(rep)], vcf)
        assert p.returncode == 0 and plain.returncode == 0, p.stderr[-400:]
        assert p.stdout == plain.stdout and p.stderr == plain.stderr
        assert rep.read_bytes().split(b"\n")[2:] == [b"examined\t0", b"kept\t0", b"dropped\t0", b""]


def test_cli_no_out_report_alone_is_a_qc_pass(bv, tmp_path):
    vcf, sets = vl.rows_vcf(257), rg.rows_sets(257)
    w = expected(bv, vcf, sets)
    rep = tmp_path / "noout.report"
    p = cli(["--noOut", "--regionFilterReport", str(rep)] + sets.cli_args(tmp_path), vcf)
    assert p.returncode == 0 and p.stdout == b"", p.stderr[-400:]
    assert rep.read_bytes() == w["report"] == sets.report([257, w["counts"][1], 257 - w["counts"][1]])
    p = cli(["--noOut"] + sets.cli_args(tmp_path), vcf)  # the regions alone make no output
    assert p.returncode == 1 and b"When specifying --noOut, must specify --dosageOutput" in p.stderr


@pytest.fixture(scope="module")
def golden(bv, golden_1kg, tmp_path_factory):
    d = tmp_path_factory.mktemp("rgg")
    vcf = golden_1kg[0]
    body, _ = oracle_side(vcf)
    (d / "g.vcf").write_bytes(vcf)
    (d / "g.bgz.vcf.gz").write_bytes(bgzf.bgzf_compress(vcf, level=1))
    out = {}
    for name, sets in zip(("third", "bed"), rg.golden_sets(body)):
        mask = rg.select(body, sets)
        out[name] = (sets, sg.kept_body(body, mask), sets.report(vl.counts(mask)))
    return d, out


@pytest.mark.parametrize("which", ["third", "bed"])
@pytest.mark.parametrize("tag,args", [("text", ["g.vcf"]), ("gzip", [GOLDEN_GZ]), ("bgzf", ["g.bgz.vcf.gz"]),
                                      ("text-2dev-batch1", ["g.vcf", "--devices", "0,0", "--batchMB", "1"]),
                                      ("bgzf-2dev-batch1", ["g.bgz.vcf.gz", "--devices", "0,0", "--batchMB", "1"])])
def test_golden_1kg(bv, golden, tmp_path, tag, args, which):
    """--regions over a third of the slice's span, and an exclude BED of 300 small intervals: the whole TSV, whatever the
    input kind, the number of workers and the batch size"""
    d, sets_of = golden
    sets, want, report = sets_of[which]
    rep = tmp_path / "rep"
    p = cli(["--in", str(d / args[0]), "--regionFilterReport", str(rep)] + sets.cli_args(tmp_path) + args[1:])
    assert p.returncode == 0, p.stderr[-400:]
    got = p.stdout.split(b"\n", 1)[1]
    assert got == want, first_diff(got, want)
    assert rep.read_bytes() == report


def test_golden_1kg_bgzf_output(bv, golden, tmp_path):
    """--compressOutput bgzf: the members inflate to the TSV of the plain run"""
    import gzip
    d, sets_of = golden
    sets, want, _ = sets_of["bed"]
    p = cli(["--in", str(d / "g.vcf"), "--compressOutput", "bgzf"] + sets.cli_args(tmp_path))
    assert p.returncode == 0, p.stderr[-400:]
    got = gzip.decompress(p.stdout).split(b"\n", 1)[1]
    assert got == want, first_diff(got, want)
