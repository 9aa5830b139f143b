"""BVCF_POISON (bvcf_devmem.h): every device and pinned buffer of a ctx filled with one byte and held between two guard zones.

A fresh allocation holds whatever the runtime hands back -- in one pytest process mostly the memory of the ctxs closed before,
or zeros -- and the kernels leave parts of their buffers unwritten on purpose: record slots without a record, the raw-list area
behind a class-map slot, census and group arrays longer than the batch, result arrays copied back in part.  A reader that
depends on such bytes shows up as nothing or as a failure that changes with the order of the tests.  Here every route through
the library runs on buffers filled with 00 (what the suite has mostly been seeing), ff (the "none" sentinels) and a5 (neither),
and every output must still be what the oracle implies -- through the helper modules of the feature tests -- with no guard
byte changed: a store that runs past an arena lands in the guard instead of the neighbouring allocation.

The inputs are the smallest the suite has for each route (`-k fill00`, `-k fillff`, `-k filla5` run one byte: ten seconds on
an MI355X).  No test here writes out of bounds: the only place where a guard is damaged on purpose is the host program of
test_devmem_cpu.py."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf
import blockcheck as bc
import closed_domains as cd
import ldpairs as lp
import mendel as md
import oracle_lib as orc
import pairtable as pt
import plinkbed as pb
import regions as rg
import samplecut
import sitegate as sg
import variantlist as vl
import vcfgen
from test_gpu_arena_growth_together import BATCH, NS, R2, T6, WINDOW, batches_of, build_input, check_files, outputs, same
from test_gpu_closed_domains import (CHAINS, CUT_SAMPLE, R_CHAINS, SITES_CHAINS, body_of, device_dosage, force, hold, kept_without,
                                     oracle, oracle_dosage, roomy_ctx, thresholds_of)
from test_gpu_names import _vcf as names_vcf
from test_gpu_sample_stats import table_from_tsv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
FILLS = ["00", "ff", "a5"]
COHORT_PIECES = ["g3-list", "g3-dense", "gg-gtdpgq"]  # 242 lines, 260 samples
SMALL_BATCH = 1 << 16  # the slots are reused by batches of different sizes


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


@pytest.fixture(scope="module", params=FILLS, ids=["fill" + f for f in FILLS])
def fill(request, bv):
    """the knob for every ctx of the module's tests, in this process and in the CLI's; the guards start clean"""
    old = os.environ.get("BVCF_POISON")
    os.environ["BVCF_POISON"] = request.param
    bv.guard_check()
    yield request.param
    if old is None:
        del os.environ["BVCF_POISON"]
    else:
        os.environ["BVCF_POISON"] = old


def no_damage(bv):
    """no guard of a live buffer, or of one freed since the last look, holds another byte than it was filled with"""
    n, msg = bv.guard_check()
    assert n == 0, "%d buffer(s) written out of bounds, the first: %s" % (n, msg)


def cli(args, data=None):
    p = subprocess.run([EXE] + args, input=data, capture_output=True, timeout=300)
    assert b"BVCF_POISON" not in p.stderr, p.stderr[-400:]  # (the CLI checks the guards before it exits)
    assert p.returncode == 0, p.stderr[-400:]
    return p


def test_the_mode_is_on(bv, fill):
    """the knob reaches the library: a ctx's buffers are listed while it lives, and none after it"""
    before = bv.guarded_buffers()  # (k_crc32's tables stay for the life of the process once made)
    ctx = bv.Ctx(9 + 260, max_batch_bytes=1 << 20)
    try:
        assert bv.guarded_buffers() >= before + 30
    finally:
        ctx.close()
    assert bv.guarded_buffers() == before
    no_damage(bv)


# ------------------------------------------------------------------ the cohort chains

@pytest.mark.parametrize("name", COHORT_PIECES)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_cohort_chains(bv, fill, monkeypatch, chain, name):
    force(monkeypatch, chain)
    hold(bv, cd.piece(name), oracle(name))
    no_damage(bv)


def test_raw_lists_behind_the_slot(bv, fill, monkeypatch):
    """2 500 samples, 16..63 non-reference lanes: the lines' entries lie behind their class-map slots where the wave has slots
    to spare, and k_gt reads them from there"""
    force(monkeypatch, "streaming")
    hold(bv, cd.piece("g3_2500-raw"), oracle("g3_2500-raw"))
    no_damage(bv)


@pytest.mark.parametrize("name", COHORT_PIECES)
def test_masked_scan(bv, fill, monkeypatch, name):
    force(monkeypatch, "streaming")
    for gq, dp in thresholds_of(name):
        want = oracle(name, (), gq, dp) if "gtdpgq" in name else oracle(name)
        hold(bv, cd.piece(name), want, {"minGQ": gq, "minDP": dp})
    no_damage(bv)


@pytest.mark.parametrize("name", COHORT_PIECES)
def test_subset_scan(bv, fill, monkeypatch, tmp_path, name):
    force(monkeypatch, "streaming")
    vcf = cd.piece(name)
    keep = samplecut.list_file(tmp_path / "keep.list", vcf[:40000], kept_without(name, CUT_SAMPLE))
    hold(bv, vcf, oracle(name, (), 0, 0, CUT_SAMPLE), {"keepSamples": keep})
    no_damage(bv)


@pytest.mark.parametrize("path", ["census", "streaming"])
@pytest.mark.parametrize("name,n_alts", [("g3-dense", 9), ("gg-gtdpgq", 11)])
def test_dosage_rows(bv, fill, monkeypatch, name, n_alts, path):
    force(monkeypatch, path)
    got, want = device_dosage(bv, cd.piece(name), n_alts), oracle_dosage(name)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert (got == want).all(), "dosage row %d differs first at sample %d" % tuple(np.argwhere(got != want)[0])
    no_damage(bv)


# ------------------------------------------------------------------ REF, ALT, POS and CHROM in small batches

@pytest.mark.parametrize("r_chain", list(R_CHAINS))
def test_r_block_with_samples(bv, fill, monkeypatch, r_chain):
    monkeypatch.setenv("BVCF_GEN_STREAM", "0")
    for k, v in R_CHAINS[r_chain].items():
        monkeypatch.setenv(k, v)
    hold(bv, cd.piece("r-single"), oracle("r-single"), max_batch_bytes=SMALL_BATCH)
    no_damage(bv)


@pytest.mark.parametrize("r_chain", ["streaming-head-walk", "streaming-head-fast"])
def test_r_block_in_long_lines(bv, fill, monkeypatch, r_chain):
    monkeypatch.setenv("BVCF_GEN_STREAM", "0")
    for k, v in R_CHAINS[r_chain].items():
        monkeypatch.setenv(k, v)
    hold(bv, cd.piece("r-pairs-long"), oracle("r-pairs-long"), max_batch_bytes=SMALL_BATCH)
    no_damage(bv)


@pytest.mark.parametrize("sites_chain", list(SITES_CHAINS))
def test_r_block_sites_only(bv, fill, monkeypatch, sites_chain):
    monkeypatch.delenv("BVCF_S2_CENSUS", raising=False)
    for k, v in SITES_CHAINS[sites_chain].items():
        monkeypatch.setenv(k, v)
    hold(bv, cd.piece("r-wordsize-sites"), oracle("r-wordsize-sites"), max_batch_bytes=SMALL_BATCH)
    no_damage(bv)


# ------------------------------------------------------------------ name lists, BGZF in, BGZF out

@functools.lru_cache(maxsize=None)
def names_case():
    names = ["S%s%d" % ("x" * (i % 13), i) for i in range(260)]
    vcf = names_vcf(337, 260, 200, names, 0.6)
    rc, out, log, _ = orc.run(vcf, {"allow": ""})
    assert rc == 0
    return vcf, out, log


def test_device_name_lists(bv, fill, monkeypatch):
    monkeypatch.setenv("BVCF_DEVICE_NAMES", "1")
    vcf, out_o, log_o = names_case()
    rc, out, log, _ = bv.run_buffer(vcf, {"allow": ""}, max_batch_bytes=SMALL_BATCH)
    assert rc == 0 and out == out_o and log == log_o
    no_damage(bv)


@functools.lru_cache(maxsize=None)
def cohort_case():
    vcf = vcfgen.gen_vcf(947, 400, 150, weird=0.02)
    rc, out, log, _ = orc.run(vcf)
    assert rc == 0
    return vcf, out, bgzf.bgzf_compress(vcf, block=777, level=1, eof_marker=True)


@pytest.mark.parametrize("window", ["0", "1", "2"])  # k_inflate's 32 KiB, 16 KiB and 4 KiB variants
def test_bgzf_input_inflated_on_the_device(bv, fill, monkeypatch, window):
    """blocks of 777 bytes: every batch starts and ends inside a line"""
    monkeypatch.setenv("BVCF_INFLATE_W16", window)
    monkeypatch.setenv("BVCF_DEVICE_INFLATE", "1")
    vcf, out_o, data = cohort_case()
    p = cli(["--batchMB", "1", "--devices", "0"], data)
    same("the TSV", p.stdout.split(b"\n", 1)[1], out_o)
    rc, got, _ = bv.bgzf_inflate_device(data)  # (the blocks alone, in this process)
    assert rc == 0 and got == vcf
    no_damage(bv)


def test_bgzf_output_deflated_on_the_device(bv, fill):
    vcf, out_o, _ = cohort_case()
    p = cli(["--compressOutput", "bgzf"], vcf)
    same("the TSV", gzip.decompress(p.stdout).split(b"\n", 1)[1], out_o)
    packed = bv.bgzf_deflate_device(out_o)  # (the compressor alone, in this process)
    assert gzip.decompress(bytes(packed)) == out_o
    no_damage(bv)


# ------------------------------------------------------------------ all analyses and gates at once, with growth

HWE = {"hwe": 0.001}
_ALL = {}


def all_case(bv):
    """test_gpu_arena_growth_together's input -- three batches of 1 MiB, one of which outruns every arena -- behind --regions,
    --excludeVariants and the site gate with --hwe, and what every output must then be: the oracle's rows with the unselected
    ones taken out (regions, variantlist, sitegate), and each analysis as the reference of its module over the rows that
    stay.  The selections are light, and the oracle's side shows that a batch still outruns each arena's starting bound."""
    if _ALL:
        return _ALL
    vcf, fam = build_input()
    names = pt.sample_names(vcf)
    rc, body, log, _ = orc.run(vcf)
    assert rc == 0
    # --regions: every chromosome from its fourth position on
    by = {}
    for r in vl.rows_of(body):
        f = r.split(b"\t")
        if rg.pos_of(f[rg.POS]) is not None:
            by.setdefault(f[rg.CHROM], set()).add(rg.pos_of(f[rg.POS]))
    sets = rg.Sets(regions=b",".join(b"%s:%d-" % (c, max(sorted(ps)[min(3, len(ps) - 1)], 1)) for c, ps in sorted(by.items())))
    rmask = rg.select(body, sets)
    left = sg.kept_body(body, rmask)
    # --excludeVariants: every 40th row the regions leave, some rows they took out, and a locus no row has
    listed = vl.loci_of(left)[::40] + vl.loci_of(sg.kept_body(body, [not m for m in rmask]))[:5] + [b"chrNone:1:A:T"]
    vmask = vl.select(left, listed, True)
    left2 = sg.kept_body(left, vmask)
    gmask, _, greport = sg.gate(left2, len(names), HWE)
    kept = sg.kept_body(left2, gmask)
    it_v = iter(vmask)
    mask = [m and next(it_v) for m in rmask]
    it_g = iter(gmask)
    mask = [m and next(it_g) for m in mask]
    assert 0 < sum(rmask) < len(rmask) and 0 < sum(vmask) < len(vmask) and 0 < sum(gmask) < len(gmask)
    assert sum(mask) > 0.9 * len(mask), "the selections are meant to be light"
    want = {"body": kept, "log": log, "plink": pb.expected_from_body(kept, names), "mendel": md.expected_from_body(kept, names, fam),
            "ld": lp.expected_from_body(kept, names, WINDOW, T6), "stats": table_from_tsv(bv, kept, names),
            "pairs": pt.file_text(pt.tables(*pt.matrices(kept, names)), names),
            "region_report": sets.report(vl.counts(rmask)), "variant_report": vl.report_text(len(set(listed)), vl.counts(vmask)),
            "site_report": greport}
    # growth, the drain and re-submission are still part of the run: per batch, the rows that stay against the starting bounds
    need_bed, need_trio, need_ld, row0, kept0 = [], [], [], 0, 0
    rows = vl.rows_of(body)
    for b in batches_of(vcf):
        rc_b, body_b, _, _ = orc.run(b)
        assert rc_b == 0
        n = body_b.count(b"\n")
        kept_b = b"".join(r + b"\n" for r, m in zip(rows[row0:row0 + n], mask[row0:row0 + n]) if m)
        n_kept = kept_b.count(b"\n")
        need_bed.append(n_kept * pb.row_bytes(NS))
        need_trio.append(len(md.expected_from_body(kept_b, names, fam, with_errors_text=False)["events"]))
        need_ld.append(len(lp.batch_events(want["ld"]["events"], kept0, kept0 + n_kept)))
        row0, kept0 = row0 + n, kept0 + n_kept
    assert row0 == len(rows) and len(need_bed) >= 3
    assert max(need_bed) > BATCH // 4 and need_bed.index(max(need_bed)) > 0, need_bed
    assert max(need_trio) > max(BATCH // 64, 1024), need_trio
    assert max(need_ld) > max(BATCH // 64, 1024), need_ld
    _ALL.update(vcf=vcf, fam=fam, want=want, sets=sets, listed=listed)
    return _ALL


@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_all_analyses_and_gates_at_once(bv, fill, tmp_path, devices):
    c = all_case(bv)
    want = c["want"]
    src = tmp_path / "in.vcf"
    src.write_bytes(c["vcf"])
    f = outputs(tmp_path, "c")
    f["ped"].write_bytes(c["fam"])
    lst = tmp_path / "c.list"
    lst.write_bytes(vl.list_text(c["listed"]))
    reports = {k: tmp_path / ("c." + k) for k in ("regionFilterReport", "variantFilterReport", "siteFilterReport")}
    p = cli(["--in", str(src), "--batchMB", "1", "--devices", devices, "--plinkOutput", str(tmp_path / "c"), "--fam", str(f["ped"]),
             "--mendel", str(f["mendel"]), "--mendelErrors", str(f["errors"]), "--ld", str(f["ld"]), "--ldPrune", str(tmp_path / "c"),
             "--ldWindow", str(WINDOW), "--ldR2", R2, "--sampleStats", str(f["stats"]), "--relatedness", str(f["pairs"]),
             "--excludeVariants", str(lst), "--variantFilterReport", str(reports["variantFilterReport"]),
             "--regionFilterReport", str(reports["regionFilterReport"])] + c["sets"].cli_args(tmp_path, "c") +
            sg.cli_args(HWE, reports["siteFilterReport"]))
    same("the TSV", p.stdout.split(b"\n", 1)[1], want["body"])
    same("--regionFilterReport", reports["regionFilterReport"].read_bytes(), want["region_report"])
    same("--variantFilterReport", reports["variantFilterReport"].read_bytes(), want["variant_report"])
    same("--siteFilterReport", reports["siteFilterReport"].read_bytes(), want["site_report"])
    check_files(tmp_path, "c", want)
    no_damage(bv)


# ------------------------------------------------------------------ a dense batch, then a sparse and shorter one on its slots

@functools.lru_cache(maxsize=None)
def turns_case():
    """(header, [(body, oracle TSV, oracle log)]): the dense lines of G3, then the first 60 of its list-mode lines -- the same
    260 samples -- and the dense ones again"""
    dense, sparse = cd.piece("g3-dense"), cd.piece("g3-list")
    hdr = dense[:dense.index(b"\n", dense.index(b"#CHROM")) + 1]
    assert sparse.startswith(hdr)
    bodies = [body_of(dense)[2], b"".join(x + b"\n" for x in body_of(sparse)[2].split(b"\n")[:60]), body_of(dense)[2]]
    out = []
    for body in bodies:
        rc, tsv, log, _ = orc.run(hdr + body)
        assert rc == 0
        out.append((body, tsv, log))
    return hdr, out


@pytest.mark.parametrize("path", [1, 2])
def test_batches_of_different_sizes_in_turn_on_one_slot(bv, fill, monkeypatch, path):
    """what the first batch left in the slot's records, lists and maps lies behind the second batch's shorter ones"""
    monkeypatch.setenv("BVCF_GEN_STREAM", "0")
    hdr, turns = turns_case()
    ctx = roomy_ctx(bv, body_of(hdr)[0], turns[0][0], 9, n_slots=1, path=path)
    try:
        assert ctx.path() == path
        for i, (body, tsv, log) in enumerate(turns):
            ctx.submit(body)
            b = ctx.collect(tsv=(body, bv.make_config({}), bc.sample_names(hdr)))
            bc.compare(tsv, log, b.tsv, b.log, "batch %d on path %d" % (i, path))
    finally:
        ctx.close()
    no_damage(bv)
