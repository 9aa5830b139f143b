"""--relatedness: the pair tables counted on the device (bvcf_pairstats.hip.h, bvcf_enable_pair_stats, bvcf_pair_stats)
and the pairwise file made from them.

The expected tables and text come from the oracle's TSV of the same bytes (pairtable.py): 0/1 matrices of the rows'
heterozygotes / homozygotes / missingGenos lists, multiplied in numpy."""
import collections
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
import samplecut
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
    """every device path that leaves class maps (as in test_gpu_sample_stats.py)"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def split_file(vcf):
    """-> (header fields, eol_chars, the data lines' bytes)"""
    at = vcf.index(b"#CHROM")
    end = vcf.index(b"\n", at)
    crlf = vcf[end - 1:end] == b"\r"
    return len(vcf[at:end - crlf].split(b"\t")), 2 if crlf else 1, vcf[end + 1:]


def blocks_of(data, limit=48 << 20):
    pos = 0
    while pos < len(data):
        end = len(data) if len(data) - pos <= limit else data.rindex(b"\n", pos, pos + limit) + 1
        yield data[pos:end]
        pos = end


def ctx_tables(bv, vcf, allow="PASS,.", **kw):
    """bvcf_pair_stats of a ctx that the file's data lines went through"""
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, allow=allow, eol_chars=eol, pair_stats=True, **kw)
    try:
        for blk in blocks_of(data):
            ctx.process(blk)
        return ctx.pair_stats()
    finally:
        ctx.close()


def run_with_pairs(bv, vcf, tmp_path, cfg=None, **kw):
    """bvcf_run_buffer with --relatedness -> (rc, TSV body, log, file bytes)"""
    path = str(tmp_path / "pairs.tsv")
    c = dict(cfg or {})
    c["relatedness"] = path
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    with open(path, "rb") as f:
        return rc, out, log, f.read()


def first_diff(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (x, y) in enumerate(zip(g, w)):
        if x != y:
            return "line %d:\n got  %r\n want %r" % (i, x[:200], y[:200])
    return "lengths %d vs %d lines" % (len(g), len(w))


def table_diff(got, want):
    bad = np.argwhere(got != want)
    if not len(bad):
        return "equal"
    t, i, j = (int(x) for x in bad[0])
    return "%d elements differ; first [%s][%d][%d]: got %d want %d" % (len(bad), "HH OC HM".split()[t], i, j, got[t, i, j], want[t, i, j])


_WANT = {}


def oracle_side(vcf, cfg):
    """(tables, file text, TSV body, log) from the oracle: computed once per input and config, shared by the device paths"""
    key = (hashlib.sha256(vcf).digest(), tuple(sorted(cfg.items())))
    if key not in _WANT:
        rc_o, out_o, log_o, _ = orc.run(vcf, cfg)
        assert rc_o == 0
        names = pt.sample_names(vcf)
        t = pt.tables(*pt.matrices(out_o, names, cfg))
        t.setflags(write=False)
        _WANT[key] = (t, pt.file_text(t, names, cfg.get("emptyField", "!")), out_o, log_o)
    return _WANT[key]


def check_both(bv, vcf, tmp_path, cfg=None):
    """raw tables through a ctx and the file through bvcf_run_buffer, against the oracle's"""
    cfg = cfg or {}
    want_t, want_text, out_o, log_o = oracle_side(vcf, cfg)
    rc, out, log, text = run_with_pairs(bv, vcf, tmp_path, cfg)
    assert rc == 0, log
    assert out == out_o and log == log_o, "the TSV / log changed with --relatedness"
    assert text == want_text, first_diff(text, want_text)
    got_t = ctx_tables(bv, vcf, allow=cfg.get("allow", "PASS,."))
    assert got_t.shape == want_t.shape and np.array_equal(got_t, want_t), table_diff(got_t, want_t)
    return want_t, want_text


# ---- table cases

@pytest.mark.parametrize("seed", [s[0] for s in pt.FUZZ])
def test_fuzz(bv, bvcf_path, tmp_path, seed):
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",",
                                          "emptyField": "NA"}
    check_both(bv, pt.fuzz_vcf(seed), tmp_path, cfg)


@pytest.mark.parametrize("ns", pt.RARE_SAMPLES)
def test_rare_carriers_lane_and_stride_edges(bv, bvcf_path, tmp_path, ns):
    check_both(bv, pt.rare_vcf(ns), tmp_path)


def record_forms(bv, b):
    forms = collections.Counter()
    for i in range(b.n_lines):
        if int(b.lines[i]["status"]) != bv.LINE_OK:
            continue
        for slot in b.record_slots(i):
            A = b.alleles[slot]
            if int(A["ac"]) and int(A["cmap_off"]) != bv.NO_CMAP:
                forms["sparse" if int(A["flags"]) & 2 else "dense"] += 1
    return forms


def test_rare_carriers_reach_both_map_forms(bv, monkeypatch):
    """the streaming path keeps rare alleles as short class lists and common ones as dense maps: the 300-sample file
    reaches both forms, as the collected records say -- so k_pr_gemm and k_pr_sparse both count there"""
    monkeypatch.setenv("BVCF_PATH", "2")
    nh, eol, data = split_file(pt.rare_vcf(300))
    ctx = bv.Ctx(nh, pair_stats=True)
    forms = record_forms(bv, ctx.process(data))
    ctx.close()
    assert forms["sparse"] > 50 and forms["dense"] > 20, forms


@pytest.mark.parametrize("n_rows", pt.TILE_ROWS)
def test_row_tile_edges(bv, monkeypatch, tmp_path, n_rows):
    """1, 63, 64, 65 and 130 dense rows: a short tile, a full one, one row into the next, two tiles and a bit"""
    for k, v in PATHS["census"].items():
        monkeypatch.setenv(k, v)
    vcf = pt.tile_vcf(n_rows)
    assert orc.run(vcf)[1].count(b"\n") == n_rows
    check_both(bv, vcf, tmp_path)


def test_short_list_at_its_limit(bv, bvcf_path, tmp_path):
    vcf = pt.short_list_limit_vcf()
    check_both(bv, vcf, tmp_path)
    if bvcf_path == "streaming":
        nh, eol, data = split_file(vcf)
        ctx = bv.Ctx(nh, pair_stats=True)
        b = ctx.process(data)
        # the first four lines carry 15, 16, 15 and 1 non-zero map bytes: short lists of 15 and 1 entries, and the
        # 16-byte row a dense map (a line's first allele record is at the line's own index)
        n_entries = []
        for i in range(4):
            A = b.alleles[i]
            assert int(b.lines[i]["status"]) == bv.LINE_OK and int(A["ac"]) > 0
            off = int(A["cmap_off"])
            n_entries.append(int(b.cmap[off:off + 4].view("<u4")[0]) if int(A["flags"]) & 2 else None)
        ctx.close()
        assert n_entries == [15, None, 15, 1], n_entries


def test_sample_that_is_never_het_prints_empty_field(bv, bvcf_path, tmp_path):
    vcf = pt.never_het_vcf()
    t, text = check_both(bv, vcf, tmp_path, {"emptyField": "NA"})
    lines = text.decode().split("\n")[1:-1]
    with_first = [ln for ln in lines if ln.startswith("S00000\t")]
    assert len(with_first) == 8 and all(ln.endswith("\tNA") for ln in with_first)
    assert not any(ln.endswith("\tNA") for ln in lines if not ln.startswith("S00000\t"))


def test_sample_missing_on_half_the_rows(bv, bvcf_path, tmp_path):
    t, text = check_both(bv, pt.half_missing_vcf(), tmp_path)
    het_het, ibs0, het1, het2, num, den = pt.derive(t, 0, 1)
    assert het1 == 30 and int(t[0][0, 0]) == 60  # sample 0 is het on all 60 rows, sample 1 called on half of them


@pytest.mark.parametrize("ns", [1, 2])
def test_one_and_two_samples(bv, bvcf_path, tmp_path, ns):
    t, text = check_both(bv, pt.tiny_vcf(ns), tmp_path)
    assert text.count(b"\n") == ns  # header line only / one pair


@pytest.fixture(scope="module")
def golden_tables(golden_1kg):
    vcf = golden_1kg[0]
    rc, body, _, _ = orc.run(vcf)
    assert rc == 0
    return pt.tables(*pt.matrices(body, pt.sample_names(vcf)))


def test_golden_1kg_tables(bv, golden_1kg, golden_tables, bvcf_path):
    """2 504 samples, 40 x 40 pair blocks, both map forms on the streaming path; maps made on the device only"""
    got = ctx_tables(bv, golden_1kg[0], want_class_maps=False)
    assert got.shape == (3, 2504, 2504)
    assert np.array_equal(got, golden_tables), table_diff(got, golden_tables)


def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


def test_golden_1kg_cli_keep_samples(bv, golden_1kg, tmp_path):
    """200 kept samples: 19 900 pairs over the kept samples, in rank space"""
    vcf = golden_1kg[0]
    idx = sorted(random.Random(77).sample(range(2504), 200))
    want_t, want_text = pt.expected(orc.run, samplecut.cut_vcf(vcf, idx))
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx)
    out = tmp_path / "pairs.tsv"
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--keepSamples", lst, "--relatedness", str(out)])
    assert p.returncode == 0, p.stderr[-400:]
    got = out.read_bytes()
    assert got.count(b"\n") == 19900 + 1
    assert got == want_text, first_diff(got, want_text)


def test_min_gq_masked_calls_are_missing(bv, bvcf_path, tmp_path):
    vcf = pt.fuzz_vcf(13)  # GT:DP:GQ, CRLF
    st = {}
    masked = gtmask.mask_vcf(vcf, 20, 0, st)
    assert st["masked"] > 1000
    want_t, want_text = oracle_side(masked, {})[:2]
    plain_t = oracle_side(vcf, {})[0]
    assert int(want_t[2].sum()) > int(plain_t[2].sum())  # more missing calls: HM grows
    rc, out, log, text = run_with_pairs(bv, vcf, tmp_path, {"minGQ": 20})
    assert rc == 0, log
    assert text == want_text, first_diff(text, want_text)


# ---- the Ctx

def batch_tables(bv, b):
    """(3, S, S) tables of one collected batch, from its class maps"""
    rows = []
    for i in range(b.n_lines):
        if int(b.lines[i]["status"]) != bv.LINE_OK:
            continue
        for slot in b.record_slots(i):
            A = b.alleles[slot]
            if int(A["ac"]) and int(A["cmap_off"]) != bv.NO_CMAP:
                rows.append(b.classes(A).copy())
    if not rows:
        return np.zeros((3, b.n_samples, b.n_samples), dtype=np.uint64)
    cls = np.stack(rows)
    return pt.tables((cls == 1).astype(np.uint8), (cls == 2).astype(np.uint8), (cls == 3).astype(np.uint8))


@pytest.mark.parametrize("path", ["1", "2"])
def test_ctx_many_batches(bv, monkeypatch, path):
    """more batches than slots, two in flight; pair_stats() is the sum of the collected batches' own maps, and reset
    starts the sum over"""
    monkeypatch.setenv("BVCF_PATH", path)
    vcf = pt.rare_vcf(300, n_lines=600, seed=31) if path == "2" else vcfgen.gen_vcf(32, 600, 40, weird=0.05)
    nh, eol, data = split_file(vcf)
    ns = nh - 9
    lines = data.split(b"\n")[:-1]
    blocks = [b"".join(x + b"\n" for x in lines[i:i + 45]) for i in range(0, len(lines), 45)]
    assert len(blocks) > 6
    ctx = bv.Ctx(nh, n_slots=2, pair_stats=True)
    total = np.zeros((3, ns, ns), dtype=np.uint64)
    since_reset = np.zeros((3, ns, ns), dtype=np.uint64)
    pending = 0
    for k, blk in enumerate(blocks):
        ctx.submit(blk, k)
        pending += 1
        if pending == 2:
            t = batch_tables(bv, ctx.collect())
            total += t
            since_reset += t
            pending -= 1
        if k == len(blocks) // 2:
            got = ctx.pair_stats(reset=True)  # (the batch still in flight is not collected: not counted yet)
            assert np.array_equal(got, since_reset), table_diff(got, since_reset)
            since_reset[:] = 0
    while pending:
        t = batch_tables(bv, ctx.collect())
        total += t
        since_reset += t
        pending -= 1
    assert np.array_equal(ctx.pair_stats(), since_reset)
    assert np.array_equal(ctx.pair_stats(reset=True), since_reset)
    assert not ctx.pair_stats().any()
    assert total[0].trace() > 0 and total[1].sum() > 0 and total[2].sum() > 0
    ctx.close()


def test_ctx_that_was_not_enabled(bv):
    ctx = bv.Ctx(9 + 4)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.pair_stats()
    assert ei.value.rc == bv.E_ARG
    ctx.close()


def test_ctx_above_the_cap(bv):
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + bv.PAIR_MAX_SAMPLES + 1, pair_stats=True, max_batch_bytes=1 << 20)
    assert ei.value.rc == bv.E_ARG and "8192" in str(ei.value)
    ctx = bv.Ctx(9, pair_stats=True)  # no sample columns: a no-op, and an empty table
    assert ctx.pair_stats().shape == (3, 0, 0)
    ctx.close()


# ---- the CLI (each run under its own time limit)

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("pr")
    vcf = vcfgen.gen_vcf(41, 3000, 400, weird=0.02) + vcfgen.gen_vcf(42, 1500, 400, weird=0.02).split(b"\n", 3)[3]
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    rc, out_o, _, _ = orc.run(vcf)
    assert rc == 0
    return vcf, paths, d, out_o, pt.expected(orc.run, vcf)[1]


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        st = d / ("%s.pairs" % tag)
        p = cli(args + ["--relatedness", str(st)], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        got = st.read_bytes()
        assert got == want, (tag, first_diff(got, want))


def test_cli_no_out_qc_pass(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    st = d / "noout.pairs"
    p = cli(["--in", str(paths["text"]), "--noOut", "--relatedness", str(st)])
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == b""
    assert st.read_bytes() == want
    # --noOut alone still needs a dosage file, with the reference's message
    p = cli(["--in", str(paths["text"]), "--noOut"])
    assert p.returncode == 1 and b"When specifying --noOut, must specify --dosageOutput" in p.stderr


def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    outs = {}
    for tag, extra in (("plain", []), ("pairs", ["--relatedness", str(d / "o.pairs")])):
        tsv, dos, smp, sst = d / ("%s.tsv.gz" % tag), d / ("%s.arrow" % tag), d / ("%s.samples" % tag), d / ("%s.stats" % tag)
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--compressOutput", "bgzf", "--dosageOutput", str(dos),
                 "--sample", str(smp), "--sampleStats", str(sst)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        outs[tag] = tuple(hashlib.sha256(f.read_bytes()).hexdigest() for f in (tsv, dos, smp, sst)) + (p.stderr,)
    assert outs["plain"] == outs["pairs"]
    assert (d / "o.pairs").read_bytes() == want


def test_cli_sites_only_unwritable_and_the_cap(bv, tmp_path):
    header_only = ("\t".join(pt.COLUMNS) + "\n").encode()
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    st = tmp_path / "sites.pairs"
    p = cli(["--relatedness", str(st)], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    assert st.read_bytes() == header_only
    bad = tmp_path / "no_such_dir" / "x.pairs"
    p = cli(["--relatedness", str(bad)], vcf)
    assert p.returncode == 1 and str(bad).encode() in p.stderr
    assert p.stdout == b""
    # one sample too many: one message, before anything is counted
    ns = 8193
    wide = (vcfgen.header(ns) + "\t".join(["chr1", "100", ".", "A", "C", "50", "PASS", ".", "GT"] + ["0|1"] * ns) + "\n").encode()
    st2 = tmp_path / "wide.pairs"
    p = cli(["--relatedness", str(st2)], wide)
    assert p.returncode == 1
    assert p.stderr.count(b"\n") == 1 and b"8193 samples" in p.stderr and b"8192" in p.stderr, p.stderr[-400:]
    assert st2.read_bytes() == b""  # (opened early, written only by a run that succeeds)
