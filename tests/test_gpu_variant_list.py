"""Row selection by a list of locus strings on the device (bvcf_variantlist.hip.h, bvcf_set_variant_list): whole runs with
--keepVariants / --excludeVariants against the oracle's run of the same bytes with the unselected rows taken out
(variantlist.select) -- the TSV, the log, the records and dosage rows, the report, and every other output as the reference
of its own module over the rows that stay.  tests/test_variant_list_cpu.py checks the inputs used here with the oracle
alone."""
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


def expected(bv, vcf, loci, exclude, cfg=None, gate=None):
    """what a run of `vcf` with the list must produce, from the oracle's run of the same bytes: computed once, shared by
    the chains.  gate: site-gate criteria that act behind the list"""
    cfg = cfg or {}
    key = (hashlib.sha256(vcf).digest(), hashlib.sha256(b"\n".join(loci)).digest(), bool(exclude), tuple(sorted(cfg.items())),
           tuple(sorted((gate or {}).items())))
    if key not in _WANT:
        out, log = oracle_side(vcf, cfg)
        names = pt.sample_names(vcf)
        mask = vl.select(out, loci, exclude, bool(names))
        body = sg.kept_body(out, mask)
        w = {"listed_body": body, "log": log, "mask": list(mask), "counts": vl.counts(mask, bool(names)), "names": names}
        w["report"] = vl.report_text(len(set(loci)), w["counts"])
        if gate:  # the list goes first: the gate examines the rows that are left, its report counts those
            gmask, gcounts, greport = sg.gate(body, len(names), gate, cfg)
            body = sg.kept_body(body, gmask)
            it = iter(gmask)
            w["mask"] = [m and next(it) for m in mask]
            w["site_report"] = greport
        w["body"] = body
        if names:
            w["stats"] = table_from_tsv(bv, body, names, cfg)
            w["pairs"] = pt.file_text(pt.tables(*pt.matrices(body, names, cfg)), names, cfg.get("emptyField", "!"))
        _WANT[key] = w
    return _WANT[key]


def write_list(tmp_path, loci, tag="list", eol=b"\n"):
    p = tmp_path / ("%s.txt" % tag)
    p.write_bytes(vl.list_text(loci, eol))
    return str(p)


def check_run(bv, vcf, loci, exclude, tmp_path, cfg=None, expect_of=None, gate=None, tag="r", **kw):
    """bvcf_run_buffer of the original bytes with the list, its report and the two tables; expect_of: the bytes the oracle
    runs (the masked or cut file of a composed case)"""
    cfg = dict(cfg or {})
    base = {k: v for k, v in cfg.items() if k not in ("minGQ", "minDP", "keepSamples", "excludeSamples")}
    w = expected(bv, vcf if expect_of is None else expect_of, loci, exclude, base, gate)
    files = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("sampleStats", "relatedness", "variantFilterReport")}
    if gate:
        files["siteFilterReport"] = str(tmp_path / ("%s.site" % tag))
    run_cfg = dict(cfg, **(gate or {}), **files)
    run_cfg["excludeVariants" if exclude else "keepVariants"] = write_list(tmp_path, loci, tag)
    rc, out, log, _ = bv.run_buffer(vcf, run_cfg, **kw)
    assert rc == 0, log
    assert out == w["body"], first_diff(out, w["body"])
    assert log == w["log"]
    got = {k: open(p, "rb").read() for k, p in files.items()}
    assert got["variantFilterReport"] == w["report"], (got["variantFilterReport"], w["report"])
    if w["names"]:
        assert got["sampleStats"] == w["stats"], first_diff(got["sampleStats"], w["stats"])
        assert got["relatedness"] == w["pairs"], first_diff(got["relatedness"], w["pairs"])
    if gate:
        assert got["siteFilterReport"] == w["site_report"], (got["siteFilterReport"], w["site_report"])
    return w


def check_records(bv, vcf, loci, exclude, cfg=None, expect_of=None, table=False, **ctx_kw):
    """the file's blocks through a ctx with the list: every examined record's ac, an .. n_miss, pad[0] and pad[1] against
    the oracle's rows and the mask, the batches' counts, and the dosage rows of the rows that stay against the oracle's"""
    cfg = cfg or {}
    ref = vcf if expect_of is None else expect_of
    w = expected(bv, ref, loci, exclude, cfg)
    out, _ = oracle_side(ref, cfg)
    S = len(w["names"])
    rows = [sg.row_counts(r.split(b"\t"), cfg) for r in vl.rows_of(out)]
    if "dosage" not in w:
        w["dosage"] = oracle_dosage_kept(ref, cfg, w["mask"])[1]
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, allow=cfg.get("allow", "PASS,."), eol_chars=eol, want_dosage=True,
                 variants=(bv.VariantTable(loci) if table else loci, exclude), **ctx_kw)
    counts = [0, 0, 0]
    examined, dosage = [], []
    for blk in blocks_of(data):
        b = ctx.process(blk)
        counts = [x + y for x, y in zip(counts, b.variant_counts)]
        assert b.gate_counts[0] == b.gate_counts[1] == b.variant_counts[1]  # the site gate's view: the kept rows, no more
        kept_slots = []
        for i in range(b.n_lines):
            if int(b.lines[i]["status"]) != bv.LINE_OK:
                continue
            for k in b.record_slots(i):
                A = b.alleles[k]
                p0, p1 = int(A["pad"][0]), int(A["pad"][1])
                assert p0 == 0 and p1 in (0, 1)
                if int(A["ac"]) == 0 and p1 == 0:
                    continue  # a row no sample carries: not examined
                assert (int(A["ac"]) == 0) == (p1 == 1), "a row the list took out has ac == 0 and pad[1] == 1"
                examined.append((int(A["ac"]), int(A["an"]), int(A["n_het"]), int(A["n_hom"]), int(A["n_miss"])))
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


# ---- every kind of row

@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("ns", [1, 5])
def test_row_kinds(bv, chain, tmp_path, ns, which):
    """SNP, multiallelic, MNP, insertions of 1 .. 300 bases, deletions of 1 .. 123, a POS printed as it stands, every CHROM
    form; the list holds half of the file's loci and, for every locus of the file, near misses in every column -- each
    locus is listed in one of the two runs and unlisted in the other, as keep and as exclude"""
    vcf = vl.kinds_vcf(ns)
    loci = vl.loci_of(oracle_side(vcf)[0])
    lst = vl.kinds_lists(loci)[which] + vl.near_misses(sorted(set(loci)))
    for exclude in (False, True):
        w = check_run(bv, vcf, lst, exclude, tmp_path, tag="x%d" % exclude)
        assert 0 < w["counts"][1] < w["counts"][0]
        check_records(bv, vcf, lst, exclude)


def test_row_kinds_crlf_list_and_duplicates(bv, tmp_path):
    """the list as a file with \\r\\n, empty lines and repeated entries: `listed` counts the distinct ones"""
    vcf = vl.kinds_vcf(5)
    loci = vl.loci_of(oracle_side(vcf)[0])
    lst = vl.kinds_lists(loci)[0]
    w = expected(bv, vcf, lst, False)
    p = tmp_path / "crlf.txt"
    p.write_bytes(b"\r\n" + vl.list_text(lst + lst[:7], b"\r\n") + b"\n\n" + lst[0])
    rep = tmp_path / "crlf.report"
    rc, out, log, _ = bv.run_buffer(vcf, {"keepVariants": str(p), "variantFilterReport": str(rep)})
    assert rc == 0 and out == w["body"] and log == w["log"]
    assert rep.read_bytes() == w["report"]


# ---- run shapes

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts_at_the_wave_edges(bv, chain, tmp_path, n):
    vcf, lst = vl.rows_vcf(n), vl.third_of(n)
    for exclude in (False, True):
        w = check_run(bv, vcf, lst, exclude, tmp_path, tag="x%d" % exclude)
        assert w["counts"][0] == n and w["counts"][2 if exclude else 1] == len(lst)
        check_records(bv, vcf, lst, exclude, table=exclude)


@pytest.fixture(scope="module")
def stride(bv):
    ctx = bv.Ctx(9 + 1)
    n = ctx.variant_gate_stride()
    ctx.close()
    assert n and n % 256 == 0
    return n


def test_one_row_more_than_a_grid_step(bv, chain, tmp_path, stride):
    """one batch whose rows outnumber k_variant_gate's threads by one: the last row is the second step of thread 0"""
    n = stride + 1
    vcf, lst = vl.rows_vcf(n, 1), vl.third_of(n) + vl.rows_loci(n)[-2:]  # (the last row, the one of the second step, is listed)
    assert len(vcf) < 48 << 20
    keep = np.zeros(n, dtype=bool)
    keep[::3] = True
    keep[-2:] = True
    for exclude in (False, True):
        w = expected(bv, vcf, lst, exclude)
        assert w["mask"] == [bool(x) for x in keep != exclude]
        p = write_list(tmp_path, lst, "big")
        rc, out, log, _ = bv.run_buffer(vcf, {"excludeVariants" if exclude else "keepVariants": p})
        assert rc == 0, log
        assert out == w["body"], first_diff(out, w["body"])
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, eol_chars=eol, variants=(lst, False), max_lines=n + 64, max_alleles=2 * n + 1024,
                 cmap_bytes=96 * n)
    b = ctx.process(data)
    got_counts = b.variant_counts  # (counted from the slot's own arrays: while the ctx lives)
    ctx.close()
    assert b.n_lines == n and (b.lines["status"] == bv.LINE_OK).all() and (b.lines["n_rec"] == 1).all()
    A = b.alleles[:n]
    assert np.array_equal(A["ac"] != 0, keep) and np.array_equal(A["pad"][:, 1] == 1, ~keep) and not A["pad"][:, 0].any()
    assert got_counts == [n, int(keep.sum()), int((~keep).sum())]


# ---- table shapes

def test_empty_list(bv, chain, tmp_path):
    vcf = vl.rows_vcf(65)
    w = check_run(bv, vcf, [], False, tmp_path, tag="keep")
    assert w["body"] == b"" and w["counts"] == [65, 0, 65]
    check_records(bv, vcf, [], False)
    w = check_run(bv, vcf, [], True, tmp_path, tag="excl")
    assert w["body"] == oracle_side(vcf)[0] and w["counts"] == [65, 65, 0]
    check_records(bv, vcf, [], True)


def test_one_entry(bv, chain, tmp_path):
    vcf = vl.rows_vcf(65)
    for exclude in (False, True):
        w = check_run(bv, vcf, [vl.rows_loci(65)[64]], exclude, tmp_path, tag="x%d" % exclude)
        assert w["counts"] == [65, 64, 1] if exclude else w["counts"] == [65, 1, 64]


def test_probe_chain_that_wraps(bv, chain, tmp_path):
    """four entries with home slot 15 of 16 (the chain 15, 0, 1, 2); the file also holds loci that walk the chain and are
    not in it"""
    listed, every = vl.wrap_case(bv)
    vcf, lst = vl.snps_vcf(every), [vl.snp_locus(p) for p in listed]
    for exclude in (False, True):
        w = check_run(bv, vcf, lst, exclude, tmp_path, tag="x%d" % exclude)
        assert w["mask"] == [(p in listed) != exclude for p in every]
        check_records(bv, vcf, lst, exclude, table=True)


def test_collision_pair(bv, chain, tmp_path):
    """the list holds A; the file holds B != A with A's tag and home slot: B goes under keep and stays under exclude"""
    listed, in_file = vl.collision_case(bv)
    a, b = vl.collision_pair(bv)
    vcf, lst = vl.snps_vcf(in_file), [vl.snp_locus(p) for p in listed]
    for exclude in (False, True):
        w = check_run(bv, vcf, lst, exclude, tmp_path, tag="x%d" % exclude)
        assert w["mask"][in_file.index(b)] == exclude and w["mask"] == [(p in listed) != exclude for p in in_file]
        check_records(bv, vcf, lst, exclude)


# ---- composition

def half_list(vcf, cfg=None):
    return vl.every_other(vl.loci_of(oracle_side(vcf, cfg)[0]))


def test_the_list_goes_before_the_site_gate(bv, chain, tmp_path):
    """the gate examines the rows the list leaves: its report is the reference's over those rows"""
    vcf = sg.case_input("sweep")
    lst = half_list(vcf)
    for exclude in (False, True):
        w = check_run(bv, vcf, lst, exclude, tmp_path, gate=sg.SWEEP, tag="x%d" % exclude)
        n_listed = w["counts"][1]
        assert w["site_report"].startswith(b"examined\t%d\n" % n_listed) and 0 < w["body"].count(b"\n") < n_listed


def test_composed_with_min_gq(bv, tmp_path):
    vcf, masked = sg.case_input("fuzz13"), sg.case_input("masked13")
    lst = half_list(masked)
    check_run(bv, vcf, lst, False, tmp_path, {"minGQ": sg.MASK_GQ}, expect_of=masked)
    check_records(bv, vcf, lst, False, expect_of=masked, min_gq=sg.MASK_GQ)


def test_composed_with_keep_samples(bv, tmp_path):
    vcf, cut = sg.case_input("rare300"), sg.case_input("cut300")
    lst = half_list(cut)
    names = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], sg.CUT_KEEP)
    check_run(bv, vcf, lst, True, tmp_path, {"keepSamples": names}, expect_of=cut)
    check_records(bv, vcf, lst, True, expect_of=cut, sample_keep=sg.CUT_KEEP)


def test_plink_fileset_holds_the_kept_rows(bv, chain, tmp_path):
    vcf = vl.kinds_vcf(5)
    lst = vl.kinds_lists(vl.loci_of(oracle_side(vcf)[0]))[0]
    w = expected(bv, vcf, lst, False)
    prefix = tmp_path / "q"
    rc, out, log, _ = bv.run_buffer(vcf, {"keepVariants": write_list(tmp_path, lst), "plinkOutput": str(prefix)})
    assert rc == 0 and out == w["body"], log
    got = pb.read_files(prefix)
    assert pb.diff(got, pb.expected_from_body(w["body"], w["names"])) == ""
    assert [ln.split(b"\t")[1] for ln in got["bim"].split(b"\n") if ln] == vl.loci_of(w["body"])


def test_mendel_counts_the_kept_rows(bv, chain, tmp_path):
    vcf, fam = vl.pedigree_case()
    lst = half_list(vcf)
    w = expected(bv, vcf, lst, True)
    want = md.expected_from_body(w["body"], w["names"], fam)
    assert int(want["counts"].sum()) > 0
    f = {k: tmp_path / k for k in ("fam", "mendel", "errors")}
    f["fam"].write_bytes(fam)
    rc, out, log, _ = bv.run_buffer(vcf, {"excludeVariants": write_list(tmp_path, lst), "fam": str(f["fam"]),
                                          "mendel": str(f["mendel"]), "mendelErrors": str(f["errors"])})
    assert rc == 0 and out == w["body"], log
    assert f["mendel"].read_bytes() == want["mendel"] and f["errors"].read_bytes() == want["errors"]


def test_ld_window_is_over_the_thinned_rows(bv, chain, tmp_path):
    vcf, window = vl.round_trip_input()
    lst = half_list(vcf)
    w = expected(bv, vcf, lst, False)
    want = lp.expected_from_body(w["body"], w["names"], 7, 200000)
    full = lp.expected_from_body(oracle_side(vcf)[0], w["names"], 7, 200000)
    assert len(want["events"]) > 10 and want["table"] != full["table"]
    f = {"ld": tmp_path / "t.ld", "ldPrune": tmp_path / "p"}
    rc, out, log, _ = bv.run_buffer(vcf, {"keepVariants": write_list(tmp_path, lst), "ld": str(f["ld"]), "ldPrune": str(f["ldPrune"]),
                                          "ldWindow": 7})
    assert rc == 0 and out == w["body"], log
    assert f["ld"].read_bytes() == want["table"]
    assert (tmp_path / "p.prune.in").read_bytes() == want["prune_in"] and (tmp_path / "p.prune.out").read_bytes() == want["prune_out"]


def test_set_variant_list_on_a_ctx(bv):
    ctx = bv.Ctx(9, variants=([b"chr1:100:A:C"], False))  # no sample columns: a no-op
    b = ctx.process(b"chr1\t100\t.\tA\tC\t50\tPASS\t.\n")
    assert b.variant_counts == [0, 0, 0]
    ctx.close()
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + 4, variants=([b"x", b""], False))
    assert ei.value.rc == bv.E_ARG
    ctx = bv.Ctx(9 + 1)  # without a list: every row is examined and kept, nothing is marked
    b = ctx.process(b"chr1\t100\t.\tA\tC\t50\tPASS\t.\tGT\t0|1\n")
    assert b.variant_counts == [1, 1, 0] and not b.alleles["pad"].any()
    ctx.close()


# ---- the CLI (each run under its own time limit)

def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


def test_cli_sites_only_comes_out_unchanged(bv, tmp_path):
    import vcfgen
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    plain = cli([], vcf)
    lst = write_list(tmp_path, half_list(vcf))
    for flag in ("--keepVariants", "--excludeVariants"):
        rep = tmp_path / "sites.report"
        p = cli([flag, lst, "--variantFilterReport", str(rep)], vcf)
        assert p.returncode == 0 and plain.returncode == 0, p.stderr[-400:]
        assert p.stdout == plain.stdout and p.stderr == plain.stderr
        assert rep.read_bytes() == vl.report_text(len(set(half_list(vcf))), [0, 0, 0])


def test_cli_no_out_report_alone_is_a_qc_pass(bv, tmp_path):
    vcf = vl.rows_vcf(257)
    lst = write_list(tmp_path, vl.third_of(257))
    rep = tmp_path / "noout.report"
    p = cli(["--noOut", "--keepVariants", lst, "--variantFilterReport", str(rep)], vcf)
    assert p.returncode == 0 and p.stdout == b"", p.stderr[-400:]
    assert rep.read_bytes() == vl.report_text(86, [257, 86, 171])
    p = cli(["--noOut", "--keepVariants", lst], vcf)  # the list alone makes no output
    assert p.returncode == 1 and b"When specifying --noOut, must specify --dosageOutput" in p.stderr


def test_cli_round_trip_through_the_prune_lists(bv, tmp_path):
    """--ldPrune writes the lists; --keepVariants P.prune.in gives the fileset of exactly those rows, in their order, and
    --excludeVariants P.prune.out the same fileset"""
    vcf, window = vl.round_trip_input()
    src = tmp_path / "in.vcf"
    src.write_bytes(vcf)
    P = tmp_path / "P"
    p = cli(["--in", str(src), "--noOut", "--ldPrune", str(P), "--ldWindow", str(window)])
    assert p.returncode == 0, p.stderr[-400:]
    pin, pout = (tmp_path / "P.prune.in").read_bytes(), (tmp_path / "P.prune.out").read_bytes()
    assert pin.count(b"\n") > 10 and pout.count(b"\n") > 10
    sets = {}
    for tag, args in (("keep", ["--keepVariants", str(P) + ".prune.in"]), ("excl", ["--excludeVariants", str(P) + ".prune.out"])):
        Q = tmp_path / ("Q" + tag)
        p = cli(["--in", str(src), "--noOut", "--plinkOutput", str(Q)] + args)
        assert p.returncode == 0, p.stderr[-400:]
        sets[tag] = pb.read_files(Q)
        assert b"".join(ln.split(b"\t")[1] + b"\n" for ln in sets[tag]["bim"].split(b"\n") if ln) == pin
    assert sets["keep"] == sets["excl"]


# ---- the golden 1KG slice

@pytest.fixture(scope="module")
def golden(bv, golden_1kg, tmp_path_factory):
    d = tmp_path_factory.mktemp("vlg")
    vcf = golden_1kg[0]
    body, _ = oracle_side(vcf)
    lst = vl.golden_list(body)
    (d / "g.vcf").write_bytes(vcf)
    (d / "g.bgz.vcf.gz").write_bytes(bgzf.bgzf_compress(vcf, level=1))
    (d / "list.txt").write_bytes(vl.list_text(lst))
    mask = vl.select(body, lst, False)
    return d, sg.kept_body(body, mask), vl.report_text(len(lst), vl.counts(mask))


@pytest.mark.parametrize("tag,args", [("text", ["g.vcf"]), ("gzip", [GOLDEN_GZ]), ("bgzf", ["g.bgz.vcf.gz"]),
                                      ("text-batch8", ["g.vcf", "--batchMB", "8"]), ("bgzf-batch8", ["g.bgz.vcf.gz", "--batchMB", "8"])])
def test_golden_1kg(bv, golden, tag, args):
    """about 10 000 entries, every other locus of the slice: the whole TSV, whatever the input kind and the batch size"""
    d, want, report = golden
    assert 9000 < want.count(b"\n") < 11000
    rep = d / (tag + ".report")
    p = cli(["--in", str(d / args[0]), "--keepVariants", str(d / "list.txt"), "--variantFilterReport", str(rep)] + args[1:])
    assert p.returncode == 0, p.stderr[-400:]
    got = p.stdout.split(b"\n", 1)[1]
    assert got == want, first_diff(got, want)
    assert rep.read_bytes() == report
