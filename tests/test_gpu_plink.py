"""--plinkOutput: the .bed rows packed on the device (bvcf_bedrows.hip.h, bvcf_enable_bed_rows, bvcf_bed_rows) and the
PREFIX.bed / .bim / .fam made from them.

The expected files come from the oracle's TSV of the same bytes (plinkbed.py); all three must be equal byte for byte, and
the TSV and the log must be the oracle's."""
import gzip
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf
import gtmask
import oracle_lib as orc
import pairtable as pt
import plinkbed as pb
import samplecut
import sitegate as sg
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")

# the four device paths that leave class maps (as in test_gpu_pair_stats.py)
PATHS = {"census": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0"},
         "streaming": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "0"},
         "streaming-general": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "1"},
         "census-wide": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0", "BVCF_WIDE": "1", "BVCF_WIDE_WIN": "1000"}}


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


@pytest.fixture(params=list(PATHS))
def bvcf_path(request, monkeypatch):
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def use_path(monkeypatch, name):
    for k, v in PATHS[name].items():
        monkeypatch.setenv(k, v)


def split_file(vcf):
    """-> (header fields, eol_chars, the data lines' bytes)"""
    at = vcf.index(b"#CHROM")
    end = vcf.index(b"\n", at)
    crlf = vcf[end - 1:end] == b"\r"
    return len(vcf[at:end - crlf].split(b"\t")), 2 if crlf else 1, vcf[end + 1:]


_WANT = {}


def oracle_side(vcf, cfg=None):
    """(files, TSV body, log) from the oracle: computed once per input and config, shared by the device paths"""
    cfg = cfg or {}
    key = (hashlib.sha256(vcf).digest(), tuple(sorted(cfg.items())))
    if key not in _WANT:
        _WANT[key] = pb.expected(orc.run, vcf, cfg)
    return _WANT[key]


def run_with_plink(bv, vcf, tmp_path, cfg=None, tag="p", **kw):
    """bvcf_run_buffer with --plinkOutput -> (rc, TSV body, log, the three files)"""
    prefix = str(tmp_path / tag)
    c = dict(cfg or {})
    c["plinkOutput"] = prefix
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    return rc, out, log, pb.read_files(prefix)


def check(bv, vcf, tmp_path, cfg=None, **kw):
    want, out_o, log_o = oracle_side(vcf, cfg)
    rc, out, log, got = run_with_plink(bv, vcf, tmp_path, cfg, **kw)
    assert rc == 0, log
    assert out == out_o and log == log_o, "the TSV / log differ from the oracle's"
    assert not pb.diff(got, want), pb.diff(got, want)
    return want


# ---- device paths

@pytest.mark.parametrize("seed", pb.FUZZ_SEEDS)
def test_fuzz(bv, bvcf_path, tmp_path, seed):
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",",
                                          "emptyField": "NA"}
    check(bv, pt.fuzz_vcf(seed), tmp_path, cfg)


@pytest.mark.parametrize("ns", pt.RARE_SAMPLES)
def test_rare_carriers(bv, bvcf_path, tmp_path, ns):
    check(bv, pt.rare_vcf(ns), tmp_path)


@pytest.mark.parametrize("ns", pb.ALIGN_SAMPLES)
def test_alignment_and_tail(bv, monkeypatch, tmp_path, ns):
    """row_bytes from 1 to 75: every S % 4, rows that start at every alignment mod 16, rows shorter than one 16-byte
    piece and rows of several; on the streaming path (short lists and dense maps) and on the census path (dense maps)"""
    vcf = pb.align_vcf(ns)
    for path in ("streaming", "census"):
        use_path(monkeypatch, path)
        want = check(bv, vcf, tmp_path)
        assert (len(want["bed"]) - 3) % pb.row_bytes(ns) == 0 and len(want["bed"]) > 3 + 16 * pb.row_bytes(ns)


@pytest.mark.parametrize("n_rows", pt.TILE_ROWS)
def test_row_count_edges(bv, monkeypatch, tmp_path, n_rows):
    vcf = pt.tile_vcf(n_rows)
    for path in ("streaming", "census"):
        use_path(monkeypatch, path)
        want = check(bv, vcf, tmp_path)
        assert len(want["bed"]) == 3 + n_rows * pb.row_bytes(70) and want["bim"].count(b"\n") == n_rows


@pytest.mark.parametrize("ns", [300, 298])
def test_short_list_at_its_limit(bv, bvcf_path, tmp_path, ns):
    """lists of 15 entries and a row of 16 non-zero map bytes; at 298 samples byte 74, which a list can name, is the
    row's partial last byte"""
    vcf = pt.short_list_limit_vcf(ns)
    check(bv, vcf, tmp_path)
    if bvcf_path == "streaming":
        nh, eol, data = split_file(vcf)
        ctx = bv.Ctx(nh, bed_rows=True)
        b = ctx.process(data)
        forms = [bool(int(b.alleles[i]["flags"]) & 2) for i in range(4)]
        ctx.close()
        assert forms == [True, False, True, True], forms


def test_short_list_names_the_partial_last_byte(bv, monkeypatch, tmp_path):
    """298 samples: a row whose only carriers are samples 296 and 297 -- its short list has one entry, the row's last byte"""
    use_path(monkeypatch, "streaming")
    ns = 298
    lines = [vcfgen.header(ns)]
    for k, (a, b) in enumerate([("0|1", "1|1"), (".|.", "0|1"), ("1|1", "0|0")]):
        gts = ["0|0"] * ns
        gts[296], gts[297] = a, b
        lines.append(pt.snp_line(100 + 10 * k, gts))
    vcf = "".join(lines).encode()
    want = check(bv, vcf, tmp_path)
    assert len(want["bed"]) == 3 + 3 * 75 and want["bed"][3 + 74] == 0b0010  # het, hom A1; the pad bits zero
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, bed_rows=True)
    b = ctx.process(data)
    assert all(int(b.alleles[i]["flags"]) & 2 for i in range(3))
    ctx.close()


def test_nothing_survives(bv, bvcf_path, tmp_path):
    vcf = pt.rare_vcf(65)
    prefix = str(tmp_path / "none")
    rc, out, log, _ = bv.run_buffer(vcf, {"plinkOutput": prefix, "minMac": 999999})
    assert rc == 0, log
    got = pb.read_files(prefix)
    assert out == b"" and got["bed"] == pb.MAGIC and got["bim"] == b""
    assert got["fam"] == pb.fam_text(pt.sample_names(vcf))


def test_golden_1kg(bv, golden_1kg, bvcf_path, tmp_path):
    """2 504 samples: rows of 626 bytes, both map forms on the streaming path"""
    want = check(bv, golden_1kg[0], tmp_path)
    assert (len(want["bed"]) - 3) % 626 == 0 and len(want["bed"]) > 3 + 626 * 10000


# ---- composition: the reference is the oracle on the masked and cut text, minus the rows the gate takes out

def test_keep_samples_min_gq_and_gate(bv, bvcf_path, tmp_path):
    vcf = gtmask.seeded(pb.MASKED)
    ns = len(pt.sample_names(vcf))
    idx = sorted(random.Random(9300).sample(range(ns), 41))  # 41 kept samples: rows of 11 bytes, one sample in the last
    criteria = {"minMac": 2, "maxMissing": 0.2}
    st = {}
    cut = samplecut.cut_vcf(gtmask.mask_vcf(vcf, 20, 0, st), idx)
    assert st["masked"] > 100
    rc_o, body, log_o, _ = orc.run(cut)
    assert rc_o == 0
    mask, counts, _ = sg.gate(body, len(idx), criteria)
    assert 0 < counts[1] < counts[0]
    kept = sg.kept_body(body, mask)
    want = pb.expected_from_body(kept, pt.sample_names(cut))
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx, eol=b"\r\n")
    cfg = dict(criteria, keepSamples=lst, minGQ=20)
    rc, out, log, got = run_with_plink(bv, vcf, tmp_path, cfg)
    assert rc == 0, log
    assert out == kept and log == log_o
    assert not pb.diff(got, want), pb.diff(got, want)
    # and the decoded rows are the lists of the surviving TSV rows
    for g, w in zip(pb.decode_bed(got["bed"], len(idx)), pt.matrices(kept, pt.sample_names(cut))):
        assert np.array_equal(g, w)


# ---- arena growth

def test_arena_growth_run_buffer(bv, bvcf_path, tmp_path):
    """~200 rows of 2 bytes per 340-byte line: the rows outrun the arena's max_batch_bytes / 4 and process_block grows it"""
    check(bv, pb.many_alts_vcf(), tmp_path, max_batch_bytes=1 << 20)


def test_arena_growth_ctx(bv, tmp_path):
    """the same through a ctx: BVCF_E_CAPACITY with the need reported, bvcf_reserve_bed_rows, the batch again"""
    vcf = pb.many_alts_vcf()
    want = oracle_side(vcf)[0]
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, max_batch_bytes=1 << 20, bed_rows=True)
    ctx.reserve(2000, 300000, 16 << 20)  # (room for everything but the rows)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.process(data)
    assert ei.value.rc == bv.E_CAPACITY
    info = ctx.bed_rows_info()
    assert info.need_bytes == len(want["bed"]) - 3 > (1 << 20) // 4 and info.n_rows == 0 and not info.rows
    ctx.reserve_bed_rows(info.need_bytes)
    ctx.process(data)
    got = ctx.bed_rows()
    ctx.close()
    assert got.shape == ((len(want["bed"]) - 3) // 2, 2) and got.tobytes() == want["bed"][3:]


def test_arena_growth_cli(bv, tmp_path):
    vcf = pb.many_alts_vcf(n_lines=4000, seed=8701)  # 1.3 MB: two batches under --batchMB 1
    assert len(vcf) > (1 << 20)
    want, out_o, _ = oracle_side(vcf)
    src = tmp_path / "many.vcf"
    src.write_bytes(vcf)
    for tag, extra in (("one", []), ("two", ["--devices", "0,0"])):
        prefix = tmp_path / tag
        p = cli(["--in", str(src), "--batchMB", "1", "--plinkOutput", str(prefix)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        got = pb.read_files(prefix)
        assert not pb.diff(got, want), (tag, pb.diff(got, want))


# ---- the Ctx

def batch_rows(bv, b):
    """the .bed rows of one collected batch, from its own class maps"""
    rows = []
    for i in range(b.n_lines):
        if int(b.lines[i]["status"]) != bv.LINE_OK:
            continue
        for slot in b.record_slots(i):
            A = b.alleles[slot]
            if int(A["ac"]):
                assert int(A["cmap_off"]) != bv.NO_CMAP
                rows.append(pb.row_of_classes(b.classes(A)))
    return b"".join(rows)


@pytest.mark.parametrize("path", ["1", "2"])
def test_ctx_many_batches(bv, monkeypatch, path):
    """more batches than slots, two in flight: bed_rows() is the batch collected last, and the batches' rows one after
    the other are the file's"""
    monkeypatch.setenv("BVCF_PATH", path)
    vcf = pt.rare_vcf(299, n_lines=600, seed=31) if path == "2" else vcfgen.gen_vcf(32, 600, 41, weird=0.05)
    want = oracle_side(vcf)[0]
    nh, eol, data = split_file(vcf)
    lines = data.split(b"\n")[:-1]
    blocks = [b"".join(x + b"\n" for x in lines[i:i + 45]) for i in range(0, len(lines), 45)]
    assert len(blocks) > 6
    ctx = bv.Ctx(nh, n_slots=2, bed_rows=True)
    rb = pb.row_bytes(nh - 9)
    got = []

    def take():
        b = ctx.collect()
        rows = ctx.bed_rows()
        info = ctx.bed_rows_info()
        assert rows.shape[1] == rb == info.row_bytes and info.need_bytes == rows.size
        assert rows.tobytes() == batch_rows(bv, b)
        got.append(rows.tobytes())

    pending = 0
    for k, blk in enumerate(blocks):
        ctx.submit(blk, k)
        pending += 1
        if pending == 2:
            take()
            pending -= 1
    while pending:
        take()
        pending -= 1
    ctx.close()
    assert b"".join(got) == want["bed"][3:]


def test_ctx_maps_stay_on_the_device(bv, monkeypatch):
    """want_class_maps off: the maps are made for the rows and never copied back"""
    monkeypatch.setenv("BVCF_PATH", "2")
    vcf = pt.rare_vcf(129)
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, want_class_maps=False, bed_rows=True)
    b = ctx.process(data)
    rows = ctx.bed_rows()
    assert len(b.cmap) == 0  # (no host copy)
    ctx.close()
    assert rows.tobytes() == oracle_side(vcf)[0]["bed"][3:]


def test_ctx_that_was_not_enabled_and_without_samples(bv):
    ctx = bv.Ctx(9 + 4)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.bed_rows_info()
    assert ei.value.rc == bv.E_ARG
    ctx.close()
    ctx = bv.Ctx(9, bed_rows=True)  # no sample columns: a no-op, and no rows
    ctx.process(b"chr1\t100\t.\tA\tC\t50\tPASS\t.\tGT\n")
    info = ctx.bed_rows_info()
    assert (info.n_rows, info.row_bytes, info.need_bytes) == (0, 0, 0) and not info.rows
    ctx.reserve_bed_rows(1 << 20)
    ctx.close()


# ---- the CLI (each run under its own time limit)

def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("plink")
    vcf = vcfgen.gen_vcf(41, 3000, 401, weird=0.02) + vcfgen.gen_vcf(42, 1500, 401, weird=0.02).split(b"\n", 3)[3]
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    want, out_o, _ = pb.expected(orc.run, vcf)
    return vcf, paths, d, out_o, want


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        prefix = d / tag
        p = cli(args + ["--plinkOutput", str(prefix)], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        got = pb.read_files(prefix)
        assert not pb.diff(got, want), (tag, pb.diff(got, want))


def test_cli_no_out_conversion_pass(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    for tag, src in (("noout-text", "text"), ("noout-bgzf", "bgzf")):
        prefix = d / tag
        p = cli(["--in", str(paths[src]), "--noOut", "--plinkOutput", str(prefix)])
        assert p.returncode == 0, p.stderr[-400:]
        assert p.stdout == b""
        got = pb.read_files(prefix)
        assert not pb.diff(got, want), (tag, pb.diff(got, want))


def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    outs = {}
    for tag, extra in (("plain", []), ("plink", ["--plinkOutput", str(d / "o")])):
        f = {k: d / ("%s.%s" % (tag, k)) for k in ("tsv.gz", "arrow", "samples", "stats", "pairs", "report")}
        p = cli(["--in", str(paths["bgzf"]), "--out", str(f["tsv.gz"]), "--compressOutput", "bgzf", "--dosageOutput", str(f["arrow"]),
                 "--sample", str(f["samples"]), "--sampleStats", str(f["stats"]), "--relatedness", str(f["pairs"]),
                 "--minMac", "3", "--siteFilterReport", str(f["report"])] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        outs[tag] = tuple(hashlib.sha256(x.read_bytes()).hexdigest() for x in f.values()) + (p.stderr,)
    assert outs["plain"] == outs["plink"]
    # (with the gate: the rows of the fileset are the rows of that TSV)
    mask, _, _ = sg.gate(out_o, 401, {"minMac": 3})
    want_gated = pb.expected_from_body(sg.kept_body(out_o, mask), pt.sample_names(vcf))
    got = pb.read_files(d / "o")
    assert not pb.diff(got, want_gated), pb.diff(got, want_gated)


def test_cli_unwritable_prefix_and_no_samples(bv, tmp_path):
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    bad = tmp_path / "no_such_dir" / "x"
    p = cli(["--plinkOutput", str(bad)], vcf)
    assert p.returncode == 1 and p.stderr.count(b"\n") == 1 and (str(bad) + ".bed").encode() in p.stderr
    assert p.stdout == b""
    prefix = tmp_path / "sites"
    plain = cli([], vcf)
    p = cli(["--plinkOutput", str(prefix)], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == plain.stdout and p.stderr == plain.stderr
    assert pb.read_files(prefix) == {"bed": pb.MAGIC, "bim": b"", "fam": b""}
