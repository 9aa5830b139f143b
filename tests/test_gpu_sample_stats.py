"""--sampleStats: the per-sample QC table counted on the device (bvcf_samplestats.hip.h, bvcf_sample_stats).

The expected table is counted here, in Python, from the oracle's TSV of the same bytes: the rows whose heterozygotes /
homozygotes / missingGenos list names a sample, and the trTv of the rows in which it is het or hom."""
import collections
import gzip
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf
import oracle_lib as orc
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def sample_names(vcf):
    for ln in vcf.split(b"\n"):
        if ln.startswith(b"#CHROM"):
            return [x.decode() for x in ln.rstrip(b"\r").split(b"\t")[9:]]
    return []


def g3(num, den):
    return "0" if num == 0 or den == 0 else "%.3G" % (num / den)


def table_from_tsv(bv, tsv_body, names, cfg=None):
    """the --sampleStats file that the TSV body (no header line) implies"""
    cfg = cfg or {}
    hdr = bv.string_header(cfg).split("\t")
    ih, io, im, it = (hdr.index(x) for x in ("heterozygotes", "homozygotes", "missingGenos", "trTv"))
    delim, empty = cfg.get("fieldDelimiter", ";"), cfg.get("emptyField", "!")
    cnt = [collections.Counter() for _ in range(5)]
    n_rows = 0
    for row in tsv_body.split(b"\n"):
        if not row:
            continue
        f = row.decode().split("\t")
        n_rows += 1
        for q, col in enumerate((ih, io, im)):
            if f[col] != empty:
                members = f[col].split(delim)
                cnt[q].update(members)
                if q < 2 and f[it] in ("1", "2"):
                    cnt[3 if f[it] == "1" else 4].update(members)
    out = ["\t".join(bv.SAMPLE_STATS_COLUMNS)]
    for nm in names:
        het, hom, miss, ts, tv = (c[nm] for c in cnt)
        out.append("\t".join([nm, str(het), str(hom), str(miss), str(ts), str(tv), g3(het, n_rows - miss),
                              g3(hom, n_rows - miss), g3(miss, n_rows), empty if tv == 0 else g3(ts, tv)]))
    return ("\n".join(out) + "\n").encode()


def run_with_stats(bv, vcf, tmp_path, cfg=None, **kw):
    """bvcf_run_buffer with --sampleStats -> (rc, TSV body, log, table bytes)"""
    path = str(tmp_path / "stats.tsv")
    c = dict(cfg or {})
    c["sampleStats"] = path
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    with open(path, "rb") as f:
        return rc, out, log, f.read()


def check_against_oracle(bv, vcf, tmp_path, cfg=None, **kw):
    rc_o, out_o, log_o, _ = orc.run(vcf, cfg)
    rc, out, log, table = run_with_stats(bv, vcf, tmp_path, cfg, **kw)
    assert rc == 0 and rc_o == 0, log
    assert out == out_o and log == log_o, "the TSV / log changed with --sampleStats"
    want = table_from_tsv(bv, out_o, sample_names(vcf), cfg)
    assert table == want, first_diff(table, want)
    return table


def first_diff(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (x, y) in enumerate(zip(g, w)):
        if x != y:
            return "line %d:\n got  %r\n want %r" % (i, x[:200], y[:200])
    return "lengths %d vs %d lines" % (len(g), len(w))


PATHS = {"census": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0"},
         "streaming": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "0"},
         "streaming-general": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "1"},
         "census-wide": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0", "BVCF_WIDE": "1", "BVCF_WIDE_WIN": "1000"}}


@pytest.fixture(params=list(PATHS))
def bvcf_path(request, monkeypatch):
    """every device path that leaves class maps: the census path, the streaming path with k_stream and with
    k_stream_gen pinned, and the census path with the regular scan split over waves (k_gt_wide)"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.fixture(scope="module")
def golden_table(bv, golden_1kg):
    vcf = golden_1kg[0]
    rc, out, log, _ = orc.run(vcf)
    assert rc == 0
    return out, log, table_from_tsv(bv, out, sample_names(vcf))


def test_golden_1kg(bv, golden_1kg, golden_table, bvcf_path, tmp_path):
    vcf = golden_1kg[0]
    out_o, log_o, want = golden_table
    rc, out, log, table = run_with_stats(bv, vcf, tmp_path)
    assert rc == 0, log
    assert out == out_o and log == log_o
    assert table == want, first_diff(table, want)
    assert len(table.split(b"\n")) == 2504 + 2


@pytest.mark.parametrize("seed,n_lines,ns,fmt_extra,weird,eol", [
    (11, 600, 17, False, 0.05, "\n"),
    (12, 500, 300, False, 0.04, "\n"),
    (13, 400, 300, True, 0.05, "\r\n"),
    (14, 300, 70, True, 0.08, "\n"),
])
def test_fuzz(bv, bvcf_path, tmp_path, seed, n_lines, ns, fmt_extra, weird, eol):
    vcf = vcfgen.gen_vcf(seed, n_lines, ns, fmt_extra, weird=weird, eol=eol)
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",",
                                          "emptyField": "NA"}
    check_against_oracle(bv, vcf, tmp_path, cfg)


def rare_vcf(seed, n_lines=400, ns=300, fmt_extra=False):
    """lines that few samples carry (a short class list on the streaming path), with common lines among them (a dense
    map): multiallelic and MNP lines, missing, haploid, polyploid and multi-digit calls, filtered and broken lines"""
    rng = random.Random(seed)
    names = ["R%04d" % i for i in range(ns)]
    out = [vcfgen.header(ns, names=names)]
    pos = 1000
    odd = ["./.", ".|.", "1", "0", "2", "0|1|1", "0/10", "1|.", "."]
    for i in range(n_lines):
        pos += rng.randint(1, 50)
        kind = rng.random()
        if kind < 0.1:
            ref, alt = "ACG", "TCA"     # MNP
        elif kind < 0.3:
            ref, alt = "A", "C,G" if kind < 0.27 else "C,G,AT"    # multiallelic (the last one mixed: a logged error)
        else:
            ref, alt = rng.choice("ACGT"), rng.choice(["C", "T", "G", "A"])
        if ref == alt:
            alt = "N" if rng.random() < 0.5 else "T" if ref != "T" else "G"
        filt = rng.choice(["PASS", "PASS", ".", "q10"])
        gts = ["0|0"] * ns
        n_alts = alt.count(",") + 1
        n_car = rng.randint(0, 6) if rng.random() < 0.85 else rng.randint(ns // 4, ns // 2)
        for _ in range(n_car):
            s = rng.randrange(ns)
            r = rng.random()
            if r < 0.2:
                gts[s] = rng.choice(odd)
            else:
                a, b = rng.randint(0, n_alts), rng.randint(0, n_alts)
                gts[s] = "%d%s%d" % (a, rng.choice("|/"), b)
        if fmt_extra:
            gts = [g + ":%d:%d" % (rng.randint(0, 99), rng.randint(0, 99)) for g in gts]
        cols = ["chr1", str(pos), ".", ref, alt, "50", filt, "DP=10", "GT:DP:GQ" if fmt_extra else "GT"] + gts
        if rng.random() < 0.01:
            cols = cols[:-1]  # too few fields
        out.append("\t".join(cols) + "\n")
    return "".join(out).encode()


@pytest.mark.parametrize("fmt_extra", [False, True])
def test_rare_carriers_both_map_forms(bv, bvcf_path, tmp_path, fmt_extra):
    vcf = rare_vcf(21 + fmt_extra, fmt_extra=fmt_extra)
    check_against_oracle(bv, vcf, tmp_path)


def test_rare_carriers_reach_the_short_lists(bv, monkeypatch):
    """the streaming path keeps rare alleles as short class lists and common ones as dense maps: the file above
    reaches both forms, as the collected records say"""
    monkeypatch.setenv("BVCF_PATH", "2")
    vcf = rare_vcf(21)
    body = vcf[vcf.index(b"\n#CHROM"):].split(b"\n", 2)[2]
    ctx = bv.Ctx(9 + 300, sample_stats=True)
    b = ctx.process(body)
    forms = collections.Counter()
    for i in range(b.n_lines):
        if int(b.lines[i]["status"]) != bv.LINE_OK:
            continue
        for slot in b.record_slots(i):
            A = b.alleles[slot]
            if int(A["ac"]) and int(A["cmap_off"]) != bv.NO_CMAP:
                forms["sparse" if int(A["flags"]) & 2 else "dense"] += 1
    assert forms["sparse"] > 50 and forms["dense"] > 5, forms
    ctx.close()


def batch_counts(bv, b):
    """(n_samples, 6) counts of one collected batch, decoded from its class maps"""
    t = np.zeros((b.n_samples, 6), dtype=np.uint64)
    for i in range(b.n_lines):
        if int(b.lines[i]["status"]) != bv.LINE_OK:
            continue
        for slot in b.record_slots(i):
            A = b.alleles[slot]
            if int(A["ac"]) == 0:
                continue
            t[:, 5] += 1
            if int(A["cmap_off"]) == bv.NO_CMAP:
                continue
            cls = b.classes(A)
            for q in range(3):
                t[:, q] += cls == q + 1
            if int(A["trtv"]) in (1, 2):
                t[:, 2 + int(A["trtv"])] += (cls == 1) | (cls == 2)
    return t


@pytest.mark.parametrize("path", ["1", "2"])
def test_ctx_many_batches(bv, monkeypatch, path):
    """more batches than slots, two in flight; sample_stats() is the sum of the collected batches' own maps, and reset
    starts the sum over"""
    monkeypatch.setenv("BVCF_PATH", path)
    vcf = rare_vcf(31, n_lines=600, ns=300) if path == "2" else vcfgen.gen_vcf(32, 600, 40, weird=0.05)
    ns = len(sample_names(vcf))
    body = vcf[vcf.index(b"\n#CHROM"):].split(b"\n", 2)[2]
    lines = body.split(b"\n")[:-1]
    blocks = [b"".join(x + b"\n" for x in lines[i:i + 45]) for i in range(0, len(lines), 45)]
    assert len(blocks) > 6
    ctx = bv.Ctx(9 + ns, n_slots=2, sample_stats=True)
    want = np.zeros((ns, 6), dtype=np.uint64)
    since_reset = np.zeros((ns, 6), dtype=np.uint64)
    keep = []
    pending = 0
    for k, blk in enumerate(blocks):
        keep.append(blk)
        ctx.submit(blk, k)
        pending += 1
        if pending == 2:
            t = batch_counts(bv, ctx.collect())
            want += t
            since_reset += t
            pending -= 1
        if k == len(blocks) // 2:
            got = ctx.sample_stats(reset=True)  # (the batch still in flight is not collected: not counted yet)
            assert np.array_equal(got, since_reset)
            since_reset[:] = 0
    while pending:
        t = batch_counts(bv, ctx.collect())
        want += t
        since_reset += t
        pending -= 1
    assert np.array_equal(ctx.sample_stats(), since_reset)
    assert np.array_equal(ctx.sample_stats(reset=True), since_reset)
    assert not ctx.sample_stats().any()
    assert want[:, 5].max() > 0 and want[:, 0].sum() > 0
    ctx.close()


def test_ctx_without_the_flag(bv):
    ctx = bv.Ctx(9 + 4)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.sample_stats()
    assert ei.value.rc == bv.E_ARG
    ctx.close()


# ---- the CLI (each run under its own time limit)

def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("ss")
    vcf = vcfgen.gen_vcf(41, 3000, 400, weird=0.02) + vcfgen.gen_vcf(42, 1500, 400, weird=0.02).split(b"\n", 3)[3]
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    return vcf, paths, d


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d = cohort
    rc, out_o, _, _ = orc.run(vcf)
    assert rc == 0
    want = table_from_tsv(bv, out_o, sample_names(vcf))
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        st = d / ("%s.stats" % tag)
        p = cli(args + ["--sampleStats", str(st)], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        got = st.read_bytes()
        assert got == want, (tag, first_diff(got, want))


def test_cli_no_out_qc_pass(bv, cohort):
    vcf, paths, d = cohort
    st = d / "noout.stats"
    p = cli(["--in", str(paths["text"]), "--noOut", "--sampleStats", str(st)])
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == b""
    rc, out_o, _, _ = orc.run(vcf)
    assert st.read_bytes() == table_from_tsv(bv, out_o, sample_names(vcf))
    # --noOut alone still needs a dosage file, with the reference's message
    p = cli(["--in", str(paths["text"]), "--noOut"])
    assert p.returncode == 1 and b"When specifying --noOut, must specify --dosageOutput" in p.stderr


def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d = cohort
    outs = {}
    for tag, extra in (("plain", []), ("stats", ["--sampleStats", str(d / "o.stats")])):
        tsv, dos = d / ("%s.tsv.gz" % tag), d / ("%s.arrow" % tag)
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--compressOutput", "bgzf", "--dosageOutput", str(dos)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        outs[tag] = (hashlib.sha256(tsv.read_bytes()).hexdigest(), hashlib.sha256(dos.read_bytes()).hexdigest(), p.stderr)
    assert outs["plain"] == outs["stats"]
    rc, out_o, _, _ = orc.run(vcf)
    assert (d / "o.stats").read_bytes() == table_from_tsv(bv, out_o, sample_names(vcf))


def test_cli_sites_only_and_unwritable(bv, cohort, tmp_path):
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    st = tmp_path / "sites.stats"
    p = cli(["--sampleStats", str(st)], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    assert st.read_bytes() == ("\t".join(bv.SAMPLE_STATS_COLUMNS) + "\n").encode()
    bad = tmp_path / "no_such_dir" / "x.stats"
    p = cli(["--sampleStats", str(bad)], vcf)
    assert p.returncode == 1 and str(bad).encode() in p.stderr
    assert p.stdout == b""
