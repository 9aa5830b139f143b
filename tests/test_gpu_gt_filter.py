"""--minGQ / --minDP: genotypes of low quality masked inside the device's genotype scan (bvcf_gtfilter.hip.h).

The oracle knows nothing of the flag; the expected output comes from an equivalence (gtmask.py):

    device run of the ORIGINAL bytes with the thresholds  ==  oracle run of the MASKED bytes without them

byte for byte for the TSV body, the log and the dosage rows; the --sampleStats table is the one the oracle's TSV of the
masked bytes implies.  test_gt_filter_cpu.py shows that the mask bites on every seeded input used here."""
import functools
import gzip
import os
import subprocess

import pytest

import bgzf
import gtmask
import oracle_lib as orc
import vcfgen
from test_gpu_sample_stats import PATHS, first_diff, run_with_stats, sample_names, table_from_tsv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


@pytest.fixture(params=list(PATHS))
def bvcf_path(request, monkeypatch):
    """the path overrides of the other device paths: a ctx with a threshold ignores them and gives one answer"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@functools.lru_cache(maxsize=None)
def expected(name, gq, dp):
    """(TSV body, log) of the oracle over the masked bytes of a seeded input"""
    m, _ = gtmask.masked(name, gq, dp)
    rc, out, log, _ = orc.run(m, gtmask.SEEDED[name][1])
    assert rc == 0
    return out, log


def with_thresholds(cfg, gq, dp):
    c = dict(cfg or {})
    c["minGQ"], c["minDP"] = gq, dp
    return c


def check(bv, vcf, cfg, gq, dp, want=None, **kw):
    """run_buffer of the original bytes with the thresholds against the oracle over the masked bytes"""
    if want is None:
        rc_o, out_o, log_o, _ = orc.run(gtmask.mask_vcf(vcf, gq, dp), cfg)
        assert rc_o == 0
        want = (out_o, log_o)
    rc, out, log, _ = bv.run_buffer(vcf, with_thresholds(cfg, gq, dp), **kw)
    assert rc == 0, log
    assert out == want[0], first_diff(out, want[0])
    assert log == want[1]
    return out


# ---- fuzz equivalence, under every path override

@pytest.mark.parametrize("gq,dp", gtmask.THRESHOLDS)
@pytest.mark.parametrize("name", list(gtmask.FUZZ))
def test_fuzz_equivalence(bv, bvcf_path, name, gq, dp):
    check(bv, gtmask.seeded(name), gtmask.SEEDED[name][1], gq, dp, expected(name, gq, dp))


def test_filtered_ctx_takes_the_census_chain(bv, bvcf_path):
    for ns in (300, 40000):
        ctx = bv.Ctx(9 + ns, min_gq=20)
        assert ctx.path() == 1
        ctx.close()
    ctx = bv.Ctx(9 + 300, min_gq=0, min_dp=0)  # thresholds off: the path is whatever it was
    assert ctx.path() == (1 if PATHS[bvcf_path]["BVCF_PATH"] == "1" else 2)
    ctx.close()


# ---- crafted FORMAT shapes

@pytest.mark.parametrize("name", list(gtmask.CRAFTED))
def test_crafted_shapes(bv, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for gq, dp in gtmask.thresholds_of(name):
        out = check(bv, vcf, cfg, gq, dp, expected(name, gq, dp))
        # many small batches, two ctxs' worth of slots: the same bytes
        assert check(bv, vcf, cfg, gq, dp, expected(name, gq, dp), max_batch_bytes=1 << 16) == out


def _tiny(fmt, rows, ns):
    hdr = vcfgen.header(ns)
    body = "".join("\t".join(["chr1", str(100 + 10 * i), ".", "A", "C", "50", "PASS", "DP=9", fmt] + list(r)) + "\n"
                   for i, r in enumerate(rows))
    return (hdr + body).encode()


def test_thresholds_at_the_boundary(bv):
    rows = [["0/1:20", "0/1:19", "1/1:21"], ["0/1:0", "0/1:1", "0/0:0"], ["0/1:999999998", "0/1:999999999", "0/0:5"],
            ["0/1:1234567890", "1/1:0999999998", "0/1:000000000"], ["0/1:19", "0/0:20", "0/0:20"]]
    vcf = _tiny("GT:GQ", rows, 3)
    for t in (20, 19, 21, 1, 2, 999999999, 999999998):
        out = check(bv, vcf, {}, t, 0)
        assert out  # (some row is always left)
    # the same values under DP, and under both keys at once
    vcf2 = _tiny("GT:DP", rows, 3)
    for t in (20, 1, 999999999):
        check(bv, vcf2, {}, 0, t)
    both = [["0/1:20:10", "0/1:19:10", "0/1:20:9"], ["1/1:0:1", "1/1:1:0", "1/1:1:1"]]
    check(bv, _tiny("GT:GQ:DP", both, 3), {}, 20, 10)
    check(bv, _tiny("GT:GQ:DP", both, 3), {}, 1, 1)
    # what the masked run of the first file says, spelled out: T = 20 keeps 20 and 21, masks 19
    rc, out, _, _ = bv.run_buffer(_tiny("GT:GQ", rows[:1], 3), {"minGQ": 20})
    f = out.split(b"\n")[0].split(b"\t")
    hdr = bv.string_header().split("\t")
    assert f[hdr.index("heterozygotes")] == b"S00000" and f[hdr.index("homozygotes")] == b"S00002"
    assert f[hdr.index("missingGenos")] == b"S00001"


def test_ctx_rejects_a_threshold_out_of_range(bv):
    for kw in ({"min_gq": 10**9}, {"min_dp": 10**9}, {"min_gq": 0xFFFFFFFF}):
        with pytest.raises(bv.BvcfError) as ei:
            bv.Ctx(9 + 4, **kw)
        assert ei.value.rc == bv.E_ARG
    bv.Ctx(9 + 4, min_gq=999999999, min_dp=999999999).close()
    rc, _, _, _ = bv.run_buffer(gtmask.seeded("alignment"), {"minGQ": 10**9})
    assert rc == bv.E_ARG


# ---- dosage

def _device_dosage_rows(bv, vcf, gq, dp, allow="PASS,."):
    """the int8 rows bvcf_collect returns for the output alleles of `vcf`, in input order"""
    hdr_at = vcf.index(b"#CHROM")
    hdr_end = vcf.index(b"\n", hdr_at)
    crlf = vcf[hdr_end - 1:hdr_end] == b"\r"
    n_header = vcf[hdr_at:hdr_end].rstrip(b"\r").count(b"\t") + 1
    ctx = bv.Ctx(n_header, allow=allow, want_dosage=True, eol_chars=2 if crlf else 1, min_gq=gq, min_dp=dp)
    b = ctx.process(vcf[hdr_end + 1:])
    ctx.close()
    rows = []
    for i in range(len(b.lines)):
        if b.lines[i]["status"] != 0:
            continue
        for k in b.record_slots(i):
            if b.alleles[k]["ac"] == 0:
                continue  # main.go:558-560
            rows.append([int(x) for x in b.dosage[k][:n_header - 9]])
    return rows


@pytest.mark.parametrize("name", ["fuzz17", "fuzz70crlf", "fuzz300", "crafted37", "crafted5crlf", "alignment"])
def test_dosage_rows(bv, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for gq, dp in gtmask.thresholds_of(name):
        want = [d for _, d in orc.run_dosage(gtmask.masked(name, gq, dp)[0], cfg)]
        got = _device_dosage_rows(bv, vcf, gq, dp, allow=cfg.get("allow", "PASS,."))
        assert len(got) == len(want)
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, "row %d: first difference at sample %d" % (r, next(i for i in range(len(w)) if g[i] != w[i]))


def _read_matrix(path):
    import pyarrow.ipc as ipc
    t = ipc.open_file(str(path)).read_all()
    cols = [t.column(i).to_pylist() for i in range(1, t.num_columns)]
    return [(locus, [c[r] for c in cols]) for r, locus in enumerate(t.column(0).to_pylist())]


def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


def test_dosage_output_file_and_cli_no_out(bv, tmp_path):
    pytest.importorskip("pyarrow")
    name, gq, dp = "crafted130", 20, 10
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    want = orc.run_dosage(gtmask.masked(name, gq, dp)[0], cfg)
    p = tmp_path / "d.arrow"
    check(bv, vcf, dict(cfg, dosageOutput=str(p)), gq, dp, expected(name, gq, dp))
    assert _read_matrix(p) == want
    p2 = tmp_path / "d2.arrow"
    r = cli(["--noOut", "--dosageOutput", str(p2), "--minGQ", str(gq), "--minDP", str(dp)], vcf)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-400:]
    assert _read_matrix(p2) == want


# ---- --sampleStats, the device name lists

@pytest.mark.parametrize("name", ["stats300", "crafted37", "fuzz70crlf"])
def test_sample_stats_follow_the_mask(bv, tmp_path, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for gq, dp in gtmask.THRESHOLDS:
        out_m, log_m = expected(name, gq, dp)
        rc, out, log, table = run_with_stats(bv, vcf, tmp_path, with_thresholds(cfg, gq, dp))
        assert rc == 0 and out == out_m and log == log_m
        want = table_from_tsv(bv, out_m, sample_names(vcf), cfg)
        assert table == want, first_diff(table, want)
    # ... and differ from the table without the mask
    assert want != table_from_tsv(bv, orc.run(vcf, cfg)[1], sample_names(vcf), cfg)


def test_device_name_lists_follow_the_mask(bv, monkeypatch):
    monkeypatch.setenv("BVCF_DEVICE_NAMES", "1")
    for name in ("fuzz300", "crafted37"):
        check(bv, gtmask.seeded(name), gtmask.SEEDED[name][1], 20, 10, expected(name, 20, 10))


# ---- the CLI

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("gtf")
    vcf = gtmask.seeded("cohort")
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    return vcf, paths, d


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d = cohort
    out_m, log_m = expected("cohort", 20, 10)
    flags = ["--minGQ", "20", "--minDP=10"]
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        p = cli(args + flags, stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_m, (tag, first_diff(p.stdout.split(b"\n", 1)[1], out_m))
        assert p.stderr.decode(errors="replace") == log_m, tag
    # one threshold at a time through the binary too
    for gq, dp in ((20, 0), (0, 10)):
        p = cli(["--in", str(paths["bgzf"]), "--minGQ", str(gq), "--minDP", str(dp)])
        assert p.returncode == 0 and p.stdout.split(b"\n", 1)[1] == expected("cohort", gq, dp)[0]
    # compressed output inflates to the same TSV
    p = cli(["--in", str(paths["bgzf"]), "--compressOutput", "bgzf"] + flags)
    assert p.returncode == 0, p.stderr[-400:]
    assert gzip.decompress(p.stdout).split(b"\n", 1)[1] == out_m


def test_cli_no_out_qc_pass(bv, cohort):
    vcf, paths, d = cohort
    st = d / "noout.stats"
    p = cli(["--in", str(paths["bgzf"]), "--noOut", "--sampleStats", str(st), "--minGQ", "20"])
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == b""
    assert st.read_bytes() == table_from_tsv(bv, expected("cohort", 20, 0)[0], sample_names(vcf))


# ---- wide cohorts: one wave per task at any sample count

def test_wide_cohort(bv):
    vcf = gtmask.seeded("wide33000")
    assert len(sample_names(vcf)) >= 32768
    for gq, dp in ((20, 0), (20, 10)):
        check(bv, vcf, {}, gq, dp, expected("wide33000", gq, dp))


# ---- what does not change

def test_thresholds_off_is_the_parent(bv, golden_1kg):
    vcf = golden_1kg[0]
    rc_o, out_o, log_o, _ = orc.run(vcf)
    rc, out, log, _ = bv.run_buffer(vcf, {"minGQ": 0, "minDP": 0})
    assert rc == 0 and out == out_o and log == log_o
    assert sorted(out.split(b"\n")[:-1]) == golden_1kg[1]
    # FORMAT is "GT" on every line of this file: a threshold masks nothing
    rc, out2, log2, _ = bv.run_buffer(vcf, {"minGQ": 20, "minDP": 10})
    assert rc == 0 and out2 == out_o and log2 == log_o


def test_sites_only_file_is_untouched(bv):
    vcf = vcfgen.header(0, with_format=False).encode() + vcfgen.gen_vcf(95, 3000, 0, weird=0.03).split(b"\n", 3)[3]
    plain = cli([], vcf)
    masked = cli(["--minGQ", "20", "--minDP", "5"], vcf)
    assert plain.returncode == 0 and masked.returncode == 0
    assert masked.stdout == plain.stdout and masked.stderr == plain.stderr and len(plain.stdout) > 10000
    rc, out, log, _ = bv.run_buffer(vcf, {"minGQ": 20})
    assert (rc, out, log) == bv.run_buffer(vcf)[:3]
    ctx = bv.Ctx(8, min_gq=20, packed_sites=True)  # no sample columns: the sites-only chain, as without a threshold
    ctx.close()
