"""--keepSamples / --excludeSamples: the sample columns that are not selected skipped inside the device's genotype scan
(bvcf_gtsubset.hip.h).

The oracle knows nothing of the flags; the expected output comes from the one rule of include/bvcf.h (samplecut.py):

    device run of the ORIGINAL bytes with the selection  ==  oracle run of the CUT bytes without it

byte for byte for the TSV body, the log and the dosage rows; the --sampleStats table is the one the oracle's TSV of the cut
bytes implies.  test_sample_subset_cpu.py shows that the cut bites on the seeded inputs used here."""
import functools
import gzip
import os
import subprocess

import pytest

import bgzf
import gtmask
import oracle_lib as orc
import samplecut
import vcfgen
from test_gpu_sample_stats import PATHS, first_diff, run_with_stats, table_from_tsv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
SMALL = list(gtmask.FUZZ) + list(gtmask.CRAFTED)


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


@pytest.fixture(params=list(PATHS))
def bvcf_path(request, monkeypatch):
    """the path overrides of the other device paths: a ctx with a selection ignores them and gives one answer"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@functools.lru_cache(maxsize=None)
def expected(name, kind, gq=0, dp=0):
    """(TSV body, log) of the oracle over the cut (and, with thresholds, masked) bytes of a seeded input"""
    src = gtmask.masked(name, gq, dp)[0] if gq or dp else gtmask.seeded(name)
    rc, out, log, _ = orc.run(samplecut.cut_vcf(src, samplecut.selection(name, kind)), gtmask.SEEDED[name][1])
    assert rc == 0
    return out, log


def names_of(vcf, indices):
    names = samplecut.sample_names(vcf)
    return [names[i].decode() for i in indices]


def check(bv, tmp_path, vcf, cfg, kept, want=None, exclude=False, **kw):
    """run_buffer of the original bytes with the selection (as --keepSamples, or as --excludeSamples naming the complement)
    against the oracle over the cut bytes"""
    if want is None:
        rc_o, out_o, log_o, _ = orc.run(samplecut.cut_vcf(vcf, kept), cfg)
        assert rc_o == 0
        want = (out_o, log_o)
    c = dict(cfg or {})
    if exclude:
        ns = len(samplecut.sample_names(vcf))
        c["excludeSamples"] = samplecut.list_file(tmp_path / "x.list", vcf, [s for s in range(ns) if s not in set(kept)])
    else:
        c["keepSamples"] = samplecut.list_file(tmp_path / "k.list", vcf, kept)
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    assert rc == 0, log
    assert out == want[0], first_diff(out, want[0])
    assert log == want[1]
    return out


# ---- fuzz and crafted equivalence, under every path override

@pytest.mark.parametrize("name", SMALL)
def test_equivalence(bv, bvcf_path, tmp_path, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for kind in samplecut.KINDS:
        check(bv, tmp_path, vcf, cfg, samplecut.selection(name, kind), expected(name, kind))


@pytest.mark.parametrize("name", SMALL)
def test_exclude_names_the_complement(bv, tmp_path, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for kind in samplecut.KINDS:
        check(bv, tmp_path, vcf, cfg, samplecut.selection(name, kind), expected(name, kind), exclude=True)


@pytest.mark.parametrize("name", SMALL)
def test_many_small_batches(bv, tmp_path, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for kind in ("half", "tenth", "ends"):
        check(bv, tmp_path, vcf, cfg, samplecut.selection(name, kind), expected(name, kind), max_batch_bytes=1 << 16)


def test_list_file_forms(bv, tmp_path):
    """CRLF, empty lines, duplicates, no newline at the end; a --sample file fed back"""
    name = "crafted37"
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    kept = samplecut.selection(name, "half")
    names = [n.encode() for n in names_of(vcf, kept)]
    p = tmp_path / "odd.list"
    p.write_bytes(b"\r\n\n" + b"\r\n".join(reversed(names)) + b"\n\n" + names[0] + b"\n" + names[-1])
    rc, out, log, _ = bv.run_buffer(vcf, dict(cfg, keepSamples=str(p)))
    assert rc == 0 and (out, log) == expected(name, "half")
    s = tmp_path / "fed.list"
    rc, out, log, _ = bv.run_buffer(vcf, dict(cfg, keepSamples=str(p), sample=str(s)))
    assert rc == 0 and s.read_bytes() == b"".join(n + b"\n" for n in names)  # the kept names only, in header order
    rc, out2, log2, _ = bv.run_buffer(vcf, dict(cfg, keepSamples=str(s)))
    assert rc == 0 and (out2, log2) == expected(name, "half")


# ---- composition with --minGQ / --minDP

@pytest.mark.parametrize("name", SMALL)
def test_composes_with_thresholds(bv, bvcf_path, tmp_path, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for kind in ("half", "tenth", "allbutone"):
        check(bv, tmp_path, vcf, dict(cfg, minGQ=20, minDP=10), samplecut.selection(name, kind), expected(name, kind, 20, 10))
    assert expected(name, "half", 20, 10)[0] != expected(name, "half")[0]  # (the mask bites on the cut file too)


# ---- dosage

def _device_dosage_rows(bv, vcf, kept, allow="PASS,.", gq=0, dp=0):
    """the int8 rows bvcf_collect returns for the output alleles of `vcf` on a ctx that keeps `kept`, in input order"""
    hdr_at = vcf.index(b"#CHROM")
    hdr_end = vcf.index(b"\n", hdr_at)
    crlf = vcf[hdr_end - 1:hdr_end] == b"\r"
    n_header = vcf[hdr_at:hdr_end].rstrip(b"\r").count(b"\t") + 1
    ctx = bv.Ctx(n_header, allow=allow, want_dosage=True, eol_chars=2 if crlf else 1, sample_keep=kept, min_gq=gq, min_dp=dp)
    b = ctx.process(vcf[hdr_end + 1:])
    ctx.close()
    assert b.n_samples == len(kept)
    rows = []
    for i in range(len(b.lines)):
        if b.lines[i]["status"] != 0:
            continue
        for k in b.record_slots(i):
            if b.alleles[k]["ac"] == 0:
                continue  # main.go:558-560
            rows.append([int(x) for x in b.dosage[k][:len(kept)]])
    return rows


@pytest.mark.parametrize("name", ["fuzz17", "fuzz70crlf", "fuzz300", "crafted37", "crafted5crlf", "alignment"])
def test_dosage_rows(bv, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for kind in ("half", "tenth", "ends"):
        want = [d for _, d in orc.run_dosage(samplecut.cut(name, kind), cfg)]
        got = _device_dosage_rows(bv, vcf, samplecut.selection(name, kind), allow=cfg.get("allow", "PASS,."))
        assert len(got) == len(want)
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, "row %d: first difference at kept sample %d" % (r, next(i for i in range(len(w)) if g[i] != w[i]))
    # with the thresholds as well
    kept = samplecut.selection(name, "half")
    want = [d for _, d in orc.run_dosage(samplecut.cut_vcf(gtmask.masked(name, 20, 10)[0], kept), cfg)]
    assert _device_dosage_rows(bv, vcf, kept, allow=cfg.get("allow", "PASS,."), gq=20, dp=10) == want


def _read_matrix(path):
    import pyarrow.ipc as ipc
    t = ipc.open_file(str(path)).read_all()
    cols = [t.column(i).to_pylist() for i in range(1, t.num_columns)]
    return t.column_names[1:], [(locus, [c[r] for c in cols]) for r, locus in enumerate(t.column(0).to_pylist())]


def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


def test_dosage_output_file(bv, tmp_path):
    pytest.importorskip("pyarrow")
    name, kind = "crafted130", "tenth"
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    kept = samplecut.selection(name, kind)
    want = orc.run_dosage(samplecut.cut(name, kind), cfg)
    p = tmp_path / "d.arrow"
    check(bv, tmp_path, vcf, dict(cfg, dosageOutput=str(p)), kept, expected(name, kind))
    cols, rows = _read_matrix(p)
    assert cols == names_of(vcf, kept) and rows == want
    p2 = tmp_path / "d2.arrow"
    r = cli(["--noOut", "--dosageOutput", str(p2), "--keepSamples", str(tmp_path / "k.list")], vcf)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-400:]
    assert _read_matrix(p2) == (cols, want)


# ---- --sampleStats, --sample, the device name lists

@pytest.mark.parametrize("name", ["stats300", "crafted37", "fuzz70crlf"])
def test_sample_stats_follow_the_selection(bv, tmp_path, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for kind in ("half", "tenth", "one"):
        kept = samplecut.selection(name, kind)
        out_c, log_c = expected(name, kind)
        c = dict(cfg, keepSamples=samplecut.list_file(tmp_path / "k.list", vcf, kept))
        rc, out, log, table = run_with_stats(bv, vcf, tmp_path, c)
        assert rc == 0 and out == out_c and log == log_c
        want = table_from_tsv(bv, out_c, names_of(vcf, kept), cfg)
        assert table == want, first_diff(table, want)
        assert table.count(b"\n") == 1 + len(kept)  # one line per kept sample


def test_sample_list_holds_the_kept_names(bv, tmp_path):
    name = "fuzz300"
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for i, (kind, exclude) in enumerate([("tenth", False), ("allbutone", True)]):
        kept = samplecut.selection(name, kind)
        p = tmp_path / ("names%d" % i)
        check(bv, tmp_path, vcf, dict(cfg, sample=str(p)), kept, expected(name, kind), exclude=exclude)
        assert p.read_text().split("\n")[:-1] == names_of(vcf, kept)


def test_device_name_lists_take_the_kept_names(bv, tmp_path, monkeypatch):
    monkeypatch.setenv("BVCF_DEVICE_NAMES", "1")
    for name in ("fuzz300", "crafted37"):
        vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
        check(bv, tmp_path, vcf, cfg, samplecut.selection(name, "half"), expected(name, "half"))
        check(bv, tmp_path, vcf, dict(cfg, minGQ=20, minDP=10), samplecut.selection(name, "tenth"),
              expected(name, "tenth", 20, 10))


# ---- wide cohorts: the rank table in LDS up to 32 768 samples, in global memory above

def test_wide_cohort(bv, tmp_path):
    vcf = gtmask.seeded("wide33000")
    ns = samplecut.n_samples("wide33000")
    assert ns >= 32768
    tenth = samplecut.selection("wide33000", "tenth")
    assert tenth[-1] >= 32768  # the selection spans the samples past the 1 024th table entry
    check(bv, tmp_path, vcf, {}, tenth, expected("wide33000", "tenth"))
    # kept samples on both sides of word and chunk boundaries, and the last column
    edges = (31, 32, 63, 64, 1023, 1024, ns - 1)
    out = check(bv, tmp_path, vcf, {}, edges)
    assert out
    check(bv, tmp_path, vcf, {"minGQ": 20, "minDP": 10}, edges,
          orc.run(samplecut.cut_vcf(gtmask.masked("wide33000", 20, 10)[0], edges))[1:3])
    check(bv, tmp_path, vcf, {}, samplecut.selection("wide33000", "allbutone"), expected("wide33000", "allbutone"))


@pytest.mark.parametrize("ns", [32768, 32769])
def test_the_last_table_that_fits_lds_and_the_first_that_does_not(bv, tmp_path, ns):
    vcf = gtmask.wide_vcf(seed=92, ns=ns, n_lines=2)
    for kept in ((0, 31, 32, 4321, 32735, 32736, ns - 2, ns - 1), tuple(range(3, ns, 7))):
        assert check(bv, tmp_path, vcf, {}, kept)


# ---- the ctx

def test_ctx_with_a_mask(bv, bvcf_path):
    for ns in (300, 40000):
        kept = list(range(5, ns, 3))
        ctx = bv.Ctx(9 + ns, sample_keep=kept)
        assert ctx.path() == 1 and ctx.n_samples == len(kept)
        ctx.close()
    ctx = bv.Ctx(9 + 300, sample_keep=None)  # no mask: the path is whatever it was
    assert ctx.path() == (1 if PATHS[bvcf_path]["BVCF_PATH"] == "1" else 2)
    ctx.close()
    for ns in (1, 300, 40000):
        with pytest.raises(bv.BvcfError) as ei:
            bv.Ctx(9 + ns, sample_keep=[])
        assert ei.value.rc == bv.E_ARG
    with pytest.raises(bv.BvcfError):
        bv.Ctx(9 + 40, sample_keep=[40, 41, 63])  # bits at or beyond n_samples are ignored: nothing is kept
    bv.Ctx(8, sample_keep=[], packed_sites=True).close()  # no sample columns: the mask is ignored


def test_ctx_of_abi_9_is_still_served(bv, monkeypatch):
    """bvcf_create takes both versions: with BVCF_ABI_VERSION (9) nothing behind min_dp is read, so the mask is ignored"""
    assert (bv.ABI_VERSION, bv.ABI_VERSION_SUBSET) == (9, 10)
    monkeypatch.setattr(bv, "ABI_VERSION_SUBSET", bv.ABI_VERSION)
    vcf = gtmask.seeded("crafted37")
    ctx = bv.Ctx(9 + 37, sample_keep=[])  # (an all-zero mask, which version 10 refuses)
    b = ctx.process(vcf[vcf.index(b"\n", vcf.index(b"#CHROM")) + 1:])
    assert b.n_samples == 37
    ctx.close()
    monkeypatch.setattr(bv, "ABI_VERSION_SUBSET", 11)
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + 37, sample_keep=[1])
    assert ei.value.rc == bv.E_ARG


def test_ctx_results_are_in_kept_rank_space(bv):
    name = "crafted37"
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    kept = samplecut.selection(name, "tenth")
    body = vcf[vcf.index(b"\n", vcf.index(b"#CHROM")) + 1:]
    ctx = bv.Ctx(9 + 37, sample_keep=kept, sample_stats=True)
    b = ctx.process(body)
    assert b.n_samples == len(kept) and b.cmap_stride == 16
    assert ctx.sample_stats().shape == (len(kept), 6)
    ctx.close()
    full = bv.Ctx(9 + 37)
    bf = full.process(body)
    full.close()
    # n_fields and the field-count verdict are the full line's; the classes of a kept sample are those of its column
    assert list(b.lines["n_fields"]) == list(bf.lines["n_fields"]) and list(b.lines["status"]) == list(bf.lines["status"])
    n_cmp = 0
    for i in range(len(b.lines)):
        if b.lines[i]["status"] != 0:
            continue
        for k in b.record_slots(i):
            got, ref = b.classes(b.alleles[k]), bf.classes(bf.alleles[k])
            assert list(got) == [ref[s] for s in kept]
            n_cmp += 1
    assert n_cmp > 100


# ---- the CLI

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("subset")
    vcf = gtmask.seeded("cohort")
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    keep = samplecut.list_file(d / "tenth.list", vcf, samplecut.selection("cohort", "tenth"))
    excl = samplecut.list_file(d / "rest.list", vcf, samplecut.complement("cohort", samplecut.selection("cohort", "tenth")))
    return vcf, paths, d, keep, excl


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, keep, excl = cohort
    out_c, log_c = expected("cohort", "tenth")
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices0", ["--in", str(paths["text"]), "--devices", "0"], None),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("batch4", ["--in", str(paths["gz"]), "--batchMB", "4"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        p = cli(args + ["--keepSamples", keep], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_c, (tag, first_diff(p.stdout.split(b"\n", 1)[1], out_c))
        assert p.stderr.decode(errors="replace") == log_c, tag
    p = cli(["--in", str(paths["bgzf"]), "--excludeSamples=" + excl])
    assert p.returncode == 0 and p.stdout.split(b"\n", 1)[1] == out_c and p.stderr.decode(errors="replace") == log_c
    # compressed output inflates to the same TSV
    p = cli(["--in", str(paths["bgzf"]), "--compressOutput", "bgzf", "--keepSamples", keep])
    assert p.returncode == 0, p.stderr[-400:]
    assert gzip.decompress(p.stdout).split(b"\n", 1)[1] == out_c
    # a QC-only pass over the kept samples
    st = d / "noout.stats"
    p = cli(["--in", str(paths["text"]), "--noOut", "--sampleStats", str(st), "--keepSamples", keep])
    assert p.returncode == 0 and p.stdout == b"", p.stderr[-400:]
    assert st.read_bytes() == table_from_tsv(bv, out_c, names_of(vcf, samplecut.selection("cohort", "tenth")))


def test_cli_errors(bv, cohort, tmp_path):
    vcf, paths, d, keep, excl = cohort
    src = ["--in", str(paths["text"])]
    unknown = tmp_path / "unknown.list"
    unknown.write_bytes(b"S00001\nNOBODY\nS00002\nNOONE\n")
    empty = tmp_path / "empty.list"
    empty.write_bytes(b"\n\r\n")
    everyone = samplecut.list_file(tmp_path / "all.list", vcf, range(len(samplecut.sample_names(vcf))))
    for tag, args, word in [("unknown name", ["--keepSamples", str(unknown)], b'"NOBODY"'),
                            ("unknown name", ["--excludeSamples", str(unknown)], b'"NOBODY"'),
                            ("empty keep list", ["--keepSamples", str(empty)], b"nothing would be left"),
                            ("everyone excluded", ["--excludeSamples", everyone], b"nothing would be left"),
                            ("unreadable list", ["--keepSamples", str(tmp_path / "missing.list")], b"missing.list"),
                            ("unreadable list", ["--excludeSamples", str(tmp_path)], b"read ")]:
        p = cli(src + args)
        assert p.returncode == 1, (tag, p.returncode, p.stderr[-400:])
        assert word in p.stderr and b"NOONE" not in p.stderr, (tag, p.stderr[-400:])
        assert p.stderr.count(b"\n") == 1, (tag, p.stderr)  # one message
    # the library call itself: BVCF_E_FATAL
    rc, out, log, _ = bv.run_buffer(vcf, {"keepSamples": str(unknown)})
    assert rc == bv.E_FATAL and out == b"" and "NOBODY" in log
    rc, _, _, _ = bv.run_buffer(vcf, {"keepSamples": keep, "excludeSamples": excl})
    assert rc == bv.E_ARG


def test_sites_only_file(bv, tmp_path):
    vcf = vcfgen.header(0, with_format=False).encode() + vcfgen.gen_vcf(96, 3000, 0, weird=0.03).split(b"\n", 3)[3]
    empty = tmp_path / "empty.list"
    empty.write_bytes(b"")
    plain = cli([], vcf)
    assert plain.returncode == 0 and len(plain.stdout) > 10000
    for flag in ("--keepSamples", "--excludeSamples"):
        p = cli([flag, str(empty)], vcf)
        assert p.returncode == 0 and p.stdout == plain.stdout and p.stderr == plain.stderr
    named = tmp_path / "named.list"
    named.write_bytes(b"S00000\n")
    p = cli(["--keepSamples", str(named)], vcf)  # no sample columns: the name is unknown
    assert p.returncode == 1 and b'"S00000"' in p.stderr and p.stdout.count(b"\n") <= 1


def test_cli_tiny_case_by_hand(bv, tmp_path):
    rows = [["0/1", "1/1", "./."], ["0/0", "0/1", "0/0"], ["1/1", "0/1", "0/1"], ["0/1", "0/0", ""]]
    vcf = (vcfgen.header(3) + "".join("\t".join(["chr1", str(100 + 10 * i), ".", "A", "C", "50", "PASS", "DP=9", "GT"] + r) + "\n"
                                       for i, r in enumerate(rows))).encode()
    lst = tmp_path / "keep.list"
    lst.write_bytes(b"S00002\nS00000\n")
    p = cli(["--keepSamples", str(lst)], vcf)
    assert p.returncode == 0 and p.stderr == b"", p.stderr
    hdr = p.stdout.split(b"\n")[0].decode().split("\t")
    got = [dict(zip(hdr, r.decode().split("\t"))) for r in p.stdout.split(b"\n")[1:-1]]
    assert [g["pos"] for g in got] == ["100", "120", "130"]  # only S00001 carries the row at 110: it is dropped
    r100, r120, r130 = got
    assert (r100["heterozygotes"], r100["homozygotes"], r100["missingGenos"]) == ("S00000", "!", "S00002")
    assert (r100["ac"], r100["an"], r100["missingness"], r100["heterozygosity"], r100["sampleMaf"]) == ("1", "2", "0.5", "1", "0.5")
    assert (r120["heterozygotes"], r120["homozygotes"], r120["missingGenos"]) == ("S00002", "S00000", "!")
    assert (r120["ac"], r120["an"], r120["missingness"], r120["sampleMaf"]) == ("3", "4", "0", "0.75")
    # the empty trailing field of the row at 130 is one allele token that matches nothing: the last column is kept
    assert (r130["heterozygotes"], r130["missingGenos"], r130["ac"], r130["an"]) == ("S00000", "!", "1", "3")
    # ... and with the last column cut it goes with it
    lst.write_bytes(b"S00000\nS00001\n")
    p = cli(["--keepSamples", str(lst)], vcf)
    assert p.stdout.split(b"\n", 1)[1] == orc.run(samplecut.cut_vcf(vcf, [0, 1]))[1]
    assert p.stdout.split(b"\n")[4].split(b"\t")[hdr.index("an")] == b"4"
