"""--ld / --ldPrune: the pairs counted on the device (bvcf_ld.hip.h, bvcf_enable_ld, bvcf_ld_stats), the seam that joins
the batches, and the three files written from them.

The expected table and lists come from the oracle's TSV of the same bytes (ldpairs.py); all three files must be equal
byte for byte, the per-batch events and edge rows equal through a ctx, and the TSV and the log must be the oracle's."""
import gzip
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf
import gtmask
import ldpairs as lp
import mendel as md
import oracle_lib as orc
import pairtable as pt
import plinkbed as pb
import samplecut
import sitegate as sg
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")

# the four device paths that leave class maps (as in test_gpu_plink.py)
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


def oracle_side(vcf, window, r2="0.2", cfg=None):
    """(expected dict, TSV body, log) from the oracle: computed once per input, window, threshold and config"""
    cfg = cfg or {}
    key = (hashlib.sha256(vcf).digest(), window, r2, tuple(sorted(cfg.items())))
    if key not in _WANT:
        _WANT[key] = lp.expected(orc.run, vcf, window, T6[r2], cfg)
    return _WANT[key]


T6 = {"0": 0, "0.2": 200000, "1": 10 ** 6, "0.333333": 333333, "0.333334": 333334, "0.5": 500000}


def run_with_ld(bv, vcf, tmp_path, window, r2="0.2", cfg=None, tag="l", **kw):
    """bvcf_run_buffer with --ld / --ldPrune -> (rc, TSV body, log, table, .prune.in, .prune.out)"""
    c = dict(cfg or {})
    c.update(ld=str(tmp_path / (tag + ".ld")), ldPrune=str(tmp_path / tag), ldWindow=window, ldR2=r2)
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    return (rc, out, log) + tuple((tmp_path / (tag + ext)).read_bytes() for ext in (".ld", ".prune.in", ".prune.out"))


def first_diff(g, w):
    n = min(len(g), len(w))
    at = next((i for i in range(n) if g[i] != w[i]), n)
    return "%d vs %d bytes, first difference at byte %d: got %r want %r" % (len(g), len(w), at, g[at:at + 60], w[at:at + 60])


def same_files(got, want):
    table, pin, pout = got
    assert table == want["table"], "--ld: " + first_diff(table, want["table"])
    assert pin == want["prune_in"], ".prune.in: " + first_diff(pin, want["prune_in"])
    assert pout == want["prune_out"], ".prune.out: " + first_diff(pout, want["prune_out"])


def check(bv, vcf, tmp_path, window, r2="0.2", cfg=None, **kw):
    want, out_o, log_o = oracle_side(vcf, window, r2, cfg)
    rc, out, log, table, pin, pout = run_with_ld(bv, vcf, tmp_path, window, r2, cfg, **kw)
    assert rc == 0, log
    assert out == out_o and log == log_o, "the TSV / log differ from the oracle's"
    same_files((table, pin, pout), want)
    return want


def row_forms(bv, b):
    """per row of a collected batch, in output order: True for a short list (BVCF_ALLELE_CMAP_SPARSE)"""
    forms = []
    for i in range(b.n_lines):
        if int(b.lines[i]["status"]) != bv.LINE_OK:
            continue
        for slot in b.record_slots(i):
            A = b.alleles[slot]
            if int(A["ac"]):
                forms.append(bool(int(A["flags"]) & 2))
    return forms


def ctx_check(bv, vcf, want, window, t6, **kw):
    """the whole file as one batch through a ctx: the batch's events and edge rows -> the rows' forms"""
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, eol_chars=eol, ld=(window, t6), **kw)
    b = ctx.process(data)
    ev, head, tail, n_rows = ctx.ld_stats()
    info = ctx.ld_info()
    forms = row_forms(bv, b)
    ctx.close()
    n = len(want["rows"])
    k = min(window, n)
    assert n_rows == n == len(forms) and info.n_edge == k and info.row_bytes == want["bed"].shape[1]
    assert info.n_events == info.need_events == len(want["events"])
    assert np.array_equal(ev, want["events"]), "the batch's events differ"
    assert np.array_equal(head, want["bed"][:k]) and np.array_equal(tail, want["bed"][n - k:]), "the edge rows differ"
    return forms


# ---- device paths

@pytest.mark.parametrize("name", ["ld40", "ld129", "ld300"])
def test_seeded_inputs(bv, bvcf_path, tmp_path, name):
    vcf, window = lp.seeded_inputs()[name]
    for r2 in ("0.2", "1"):
        want = check(bv, vcf, tmp_path, window, r2)
        ctx_check(bv, vcf, want, window, T6[r2])
        assert len(want["events"]) > 0 and want["prune_out"]


def test_fuzz_lines(bv, bvcf_path, tmp_path):
    """vcfgen's lines: multiallelic, indels, odd genotypes, filtered lines; other TSV settings"""
    vcf = vcfgen.gen_vcf(61, 400, 37, weird=0.03)
    want = check(bv, vcf, tmp_path, 30, "0", {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",", "emptyField": "NA"})
    assert len(want["events"]) > 100
    check(bv, vcf, tmp_path, 30, "0.2", {"allow": ""})


def test_both_map_forms_in_one_pair(bv, monkeypatch, tmp_path):
    """short lists at their limit of 15 entries next to dense rows, a listed byte in the partial last byte (S = 299)"""
    use_path(monkeypatch, "streaming")
    vcf = pt.short_list_limit_vcf(300)
    want = check(bv, vcf, tmp_path, 50, "0")
    forms = ctx_check(bv, vcf, want, 50, 0)
    assert forms[:4] == [True, False, True, True], forms[:4]
    pairs = {(b - d, b) for b, d in want["events"][:, :2].tolist()}
    assert any(forms[a] != forms[b] for a, b in pairs) and any(forms[a] and forms[b] for a, b in pairs)
    rng = random.Random(8200)
    out = [vcfgen.header(299)]
    for k in range(30):
        gts = ["0|0"] * 299
        for s in rng.sample(range(290, 299), rng.randint(1, 4)) + rng.sample(range(299), 2):
            gts[s] = rng.choice(["0|1", "1|1", ".|.", "1|0"])
        out.append(pt.snp_line(100 + 10 * k, gts))
    vcf = "".join(out).encode()
    want = check(bv, vcf, tmp_path, 50, "0", tag="last")
    assert all(ctx_check(bv, vcf, want, 50, 0)) and len(want["events"]) > 20


# ---- shapes

@pytest.mark.parametrize("ns", lp.GPU_SAMPLES)
def test_cohort_sizes(bv, monkeypatch, tmp_path, ns):
    """word, lane and chunk edges of a row, a partial last byte; S = 1: no pair, every row kept"""
    vcf = lp.ld_vcf(7100 + ns, ns, 70)
    for path, window in (("streaming", 50), ("census", 7)):
        use_path(monkeypatch, path)
        want = check(bv, vcf, tmp_path, window, "0.2", tag=path)
        ctx_check(bv, vcf, want, window, 200000)
        if ns == 1:
            assert len(want["events"]) == 0 and want["prune_out"] == b""
        elif ns > 3:
            assert len(want["events"]) > 0


def test_more_than_one_chunk_of_samples(bv, monkeypatch, tmp_path):
    """S = 600 and 1 100: a row spans two and three stages of 512 samples"""
    use_path(monkeypatch, "streaming")
    for ns in (600, 1100):
        vcf = lp.ld_vcf(7200 + ns, ns, 40, carrier=0.02)
        want = check(bv, vcf, tmp_path, 50, "0.2", tag=str(ns))
        ctx_check(bv, vcf, want, 50, 200000)
        assert len(want["events"]) > 10


@pytest.mark.parametrize("n_rows", lp.GPU_ROWS)
def test_row_counts(bv, monkeypatch, tmp_path, n_rows):
    """tile edges (16 rows a workgroup, 4 a wave), rows < window"""
    vcf = lp.ld_vcf(7300 + n_rows, 23, n_rows, specials=False)
    use_path(monkeypatch, "streaming")
    for window in (1, 64, 200):
        want = check(bv, vcf, tmp_path, window, "0.2", tag=str(window))
        ctx_check(bv, vcf, want, window, 200000)
        assert len(want["rows"]) == n_rows


@pytest.mark.parametrize("window", lp.GPU_WINDOWS)
def test_windows(bv, monkeypatch, tmp_path, window):
    """partner-group edges at 64; 700 rows: windows shorter and longer than the groups, 512 = eight groups"""
    vcf = lp.ld_vcf(7400, 20, 700, specials=False)
    use_path(monkeypatch, "streaming")
    want = check(bv, vcf, tmp_path, window, "0.5")
    ctx_check(bv, vcf, want, window, 500000)
    d = want["events"][:, 1]
    assert d.max() <= window and (window < 3 or d.max() > window // 2)


@pytest.mark.parametrize("r2", ["0", "0.2", "1", "0.333333", "0.333334"])
def test_thresholds(bv, tmp_path, r2):
    vcf, window = lp.seeded_inputs()["ld40"]
    want = check(bv, vcf, tmp_path, window, r2)
    assert len(want["events"]) > 0
    ex = lp.exact_third_vcf()
    want = check(bv, ex, tmp_path, 50, r2, tag="ex")
    assert len(want["events"]) == (1 if r2 in ("0", "0.2", "0.333333") else 0)


def test_no_sample_columns_and_one_sample(bv, bvcf_path, tmp_path):
    sites = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    rc, out, log, table, pin, pout = run_with_ld(bv, sites, tmp_path, 50, tag="sites")
    assert rc == 0 and (table, pin, pout) == (lp.HEADER, b"", b"")
    assert (out, log) == orc.run(sites)[1:3]
    one = lp.ld_vcf(7500, 1, 40)
    want = check(bv, one, tmp_path, 50, "0", tag="one")
    assert want["table"] == lp.HEADER and want["prune_out"] == b"" and want["prune_in"].count(b"\n") == len(want["rows"])
    nh, eol, data = split_file(sites)
    ctx = bv.Ctx(nh, ld=(50, 200000))  # no sample columns: nothing allocated or launched
    ctx.process(data)
    info = ctx.ld_info()
    assert (info.n_events, info.need_events, info.n_rows, info.n_edge) == (0, 0, 0, 0) and not info.events
    ctx.reserve_ld_events(1 << 20)
    ctx.close()


def test_enable_ld_refuses_bad_arguments(bv):
    for bad in ((0, 0), (513, 0), (50, 10 ** 6 + 1)):
        with pytest.raises(bv.BvcfError) as ei:
            bv.Ctx(9 + 4, ld=bad)
        assert ei.value.rc == bv.E_ARG
    ctx = bv.Ctx(9 + 4)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.ld_info()
    assert ei.value.rc == bv.E_ARG
    ctx.close()


# ---- composition: the reference is the oracle on the masked and cut text, minus the rows the gate takes out

def test_keep_samples_min_gq_and_gate(bv, bvcf_path, tmp_path):
    vcf = gtmask.seeded(pb.MASKED)
    ns = len(pt.sample_names(vcf))
    idx = sorted(random.Random(9300).sample(range(ns), 41))
    criteria = {"minMac": 2, "maxMissing": 0.2}
    cut = samplecut.cut_vcf(gtmask.mask_vcf(vcf, 20, 0, {}), idx)
    rc_o, body, log_o, _ = orc.run(cut)
    assert rc_o == 0
    mask, counts, _ = sg.gate(body, len(idx), criteria)
    assert 0 < counts[1] < counts[0]
    kept = sg.kept_body(body, mask)
    want = lp.expected_from_body(kept, pt.sample_names(cut), 50, 200000)
    assert len(want["events"]) > 0
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx, eol=b"\r\n")
    cfg = dict(criteria, keepSamples=lst, minGQ=20)
    rc, out, log, table, pin, pout = run_with_ld(bv, vcf, tmp_path, 50, "0.2", cfg)
    assert rc == 0, log
    assert out == kept and log == log_o
    same_files((table, pin, pout), want)


def test_with_and_without_plink_output_and_mendel(bv, bvcf_path, tmp_path):
    """the row index and the .bed rows are made once: the fileset and the --mendel files are what they are without --ld,
    the three LD files what they are without the others -- apart, in pairs and all together"""
    vcf, trios = md.pedigree_vcf(129, 40, 100, 9860)
    fam = tmp_path / "p.fam"
    fam.write_bytes(md.fam_of(trios, pt.sample_names(vcf)))
    want = check(bv, vcf, tmp_path, 50, "0.2")
    want_p = pb.expected(orc.run, vcf)[0]
    want_m = md.expected(orc.run, vcf, fam.read_bytes())[0]
    for tag, extra in (("p", {"plinkOutput": str(tmp_path / "set_p")}),
                       ("m", {"fam": str(fam), "mendel": str(tmp_path / "m.mendel"), "mendelErrors": str(tmp_path / "m.errors")}),
                       ("pm", {"plinkOutput": str(tmp_path / "set_pm"), "fam": str(fam), "mendel": str(tmp_path / "pm.mendel"),
                               "mendelErrors": str(tmp_path / "pm.errors")})):
        rc, out, log, table, pin, pout = run_with_ld(bv, vcf, tmp_path, 50, "0.2", extra, tag="with_" + tag)
        assert rc == 0, log
        same_files((table, pin, pout), want)
        if "p" in tag:
            assert not pb.diff(pb.read_files(tmp_path / ("set_" + tag)), want_p)
        if "m" in tag:
            assert (tmp_path / (tag + ".mendel")).read_bytes() == want_m["mendel"]
            assert (tmp_path / (tag + ".errors")).read_bytes() == want_m["errors"]
    # and through a ctx with all three enabled
    ctx_check(bv, vcf, want, 50, 200000, bed_rows=True, trios=want_m["trios"])


def test_one_output_at_a_time(bv, monkeypatch, tmp_path):
    use_path(monkeypatch, "streaming")
    vcf, window = lp.seeded_inputs()["ld40"]
    want, body, _ = oracle_side(vcf, window)
    rc, out, log, _ = bv.run_buffer(vcf, {"ld": str(tmp_path / "only.ld"), "ldWindow": window})
    assert rc == 0 and out == body and (tmp_path / "only.ld").read_bytes() == want["table"]
    rc, out, log, _ = bv.run_buffer(vcf, {"ldPrune": str(tmp_path / "only"), "ldWindow": window})
    assert rc == 0 and out == body
    assert (tmp_path / "only.prune.in").read_bytes() == want["prune_in"] and (tmp_path / "only.prune.out").read_bytes() == want["prune_out"]
    assert sorted(os.listdir(tmp_path)) == ["only.ld", "only.prune.in", "only.prune.out"]


# ---- arena growth: a threshold of 0 over a long window

def growth_vcf(n_rows=400):
    return lp.ld_vcf(7600, 12, n_rows, specials=False, miss=0.0, carrier=0.5)


def test_arena_growth_run_buffer(bv, bvcf_path, tmp_path):
    vcf = growth_vcf()
    want = check(bv, vcf, tmp_path, 512, "0", max_batch_bytes=1 << 20)
    assert len(want["events"]) > (1 << 20) // 64


def test_arena_growth_ctx(bv):
    """BVCF_E_CAPACITY with the need reported, bvcf_reserve_ld_events, the batch again"""
    vcf = growth_vcf()
    want = oracle_side(vcf, 512, "0")[0]
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, max_batch_bytes=1 << 20, ld=(512, 0))
    with pytest.raises(bv.BvcfError) as ei:
        ctx.process(data)
    assert ei.value.rc == bv.E_CAPACITY
    info = ctx.ld_info()
    assert info.need_events == len(want["events"]) and info.n_events == 0 and not info.events
    ctx.reserve_ld_events(info.need_events)
    ctx.process(data)
    ev, head, tail, n_rows = ctx.ld_stats()
    ctx.close()
    assert np.array_equal(ev, want["events"])


def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


def ld_args(d, tag, window=50, r2="0.2"):
    return ["--ld", str(d / (tag + ".ld")), "--ldPrune", str(d / tag), "--ldWindow", str(window), "--ldR2", r2]


def read_ld(d, tag):
    return tuple((d / (tag + ext)).read_bytes() for ext in (".ld", ".prune.in", ".prune.out"))


def test_arena_growth_cli(bv, tmp_path):
    vcf = growth_vcf(1200)
    want, out_o, _ = oracle_side(vcf, 200, "0")
    assert len(want["events"]) > 100000
    src = tmp_path / "e.vcf"
    src.write_bytes(vcf)
    for tag, extra in (("one", []), ("two", ["--devices", "0,0"])):
        p = cli(["--in", str(src), "--batchMB", "1"] + ld_args(tmp_path, tag, 200, "0") + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        same_files(read_ld(tmp_path, tag), want)


# ---- the Ctx

@pytest.mark.parametrize("path", ["1", "2"])
def test_ctx_many_batches(bv, monkeypatch, path):
    """more batches than slots, two in flight, batches shorter than the window: ld_stats() is the batch collected last;
    the batches through the seam give the file's table and lists"""
    monkeypatch.setenv("BVCF_PATH", path)
    vcf = lp.ld_vcf(7700, 75, 600)
    window = 64
    want = oracle_side(vcf, window)[0]
    nh, eol, data = split_file(vcf)
    lines = data.split(b"\n")[:-1]
    cuts = [0, 45, 46, 50, 110, 300, 301, 420, len(lines)]
    blocks = [b"".join(x + b"\n" for x in lines[lo:hi]) for lo, hi in zip(cuts, cuts[1:])]
    ctx = bv.Ctx(nh, n_slots=2, ld=(window, 200000), want_class_maps=False)
    seam = bv.LdSeam(75, window, 200000)
    loci = lp.loci_of(want["rows"])
    row0 = 0

    def take():
        nonlocal row0
        b = ctx.collect()
        assert len(b.cmap) == 0  # (the maps stay on the device)
        ev, head, tail, n_rows = ctx.ld_stats()
        assert n_rows == len(row_forms(bv, b))
        assert np.array_equal(ev, lp.batch_events(want["events"], row0, row0 + n_rows))
        seam.push_edges(n_rows, head, tail, ev, loci[row0:row0 + n_rows])
        row0 += n_rows

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
    assert lp.HEADER + seam.read(0) == want["table"]
    assert (seam.read(1), seam.read(2)) == (want["prune_in"], want["prune_out"])
    seam.close()


# ---- the CLI (each run under its own time limit)

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("ld")
    vcf = lp.ld_vcf(7800, 401, 2600, carrier=0.05)
    assert len(vcf) > 3 << 20
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    want, out_o, _ = lp.expected(orc.run, vcf, 50, 200000)
    return vcf, paths, d, out_o, want


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    assert len(want["events"]) > 1000
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        p = cli(args + ld_args(d, tag), stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        same_files(read_ld(d, tag), want)


def test_cli_no_out_qc_pass(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    for tag, src in (("noout-text", "text"), ("noout-bgzf", "bgzf")):
        p = cli(["--in", str(paths[src]), "--noOut"] + ld_args(d, tag))
        assert p.returncode == 0, p.stderr[-400:]
        assert p.stdout == b""
        same_files(read_ld(d, tag), want)
    p = cli(["--in", str(paths["text"]), "--noOut", "--ldPrune", str(d / "lists-only")])
    assert p.returncode == 0 and (d / "lists-only.prune.in").read_bytes() == want["prune_in"]
    p = cli(["--in", str(paths["text"]), "--noOut", "--ldWindow", "20", "--ldR2", "0.5"])  # the two numbers alone: no QC pass
    assert p.returncode == 1 and b"noOut" in p.stderr


def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    names = md.normalized(pt.sample_names(vcf))
    fam = d / "c.fam"
    fam.write_bytes(md.fam_of(md.random_trios(401, 50, 9890), names))
    outs = {}
    for tag, extra in (("plain", []), ("numbers-only", ["--ldWindow", "7", "--ldR2", "0.5"]), ("ld", ld_args(d, "o"))):
        f = {k: d / ("%s.%s" % (tag, k)) for k in ("tsv.gz", "arrow", "samples", "stats", "pairs", "report", "mendel", "errors")}
        prefix = d / ("%s.plink" % tag)
        p = cli(["--in", str(paths["bgzf"]), "--out", str(f["tsv.gz"]), "--compressOutput", "bgzf", "--dosageOutput", str(f["arrow"]),
                 "--sample", str(f["samples"]), "--sampleStats", str(f["stats"]), "--relatedness", str(f["pairs"]),
                 "--minMac", "3", "--siteFilterReport", str(f["report"]), "--plinkOutput", str(prefix), "--fam", str(fam),
                 "--mendel", str(f["mendel"]), "--mendelErrors", str(f["errors"])] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        outs[tag] = tuple(hashlib.sha256(x.read_bytes()).hexdigest() for x in f.values()) + \
            tuple(hashlib.sha256(x).hexdigest() for x in pb.read_files(prefix).values()) + (p.stderr,)
    assert outs["plain"] == outs["numbers-only"] == outs["ld"]
    # (with the gate: the rows paired are the rows of that TSV, and the lists name the rows of that .bim)
    mask, _, _ = sg.gate(out_o, 401, {"minMac": 3})
    gated = lp.expected_from_body(sg.kept_body(out_o, mask), pt.sample_names(vcf), 50, 200000)
    same_files(read_ld(d, "o"), gated)
    bim = [ln.split(b"\t")[1] for ln in pb.read_files(d / "ld.plink")["bim"].split(b"\n") if ln]
    assert sorted(bim) == sorted((gated["prune_in"] + gated["prune_out"]).split(b"\n")[:-1])


def test_cli_flag_errors(bv, tmp_path):
    vcf, window = lp.seeded_inputs()["ld40"]
    for args in (["--ld"], ["--ldPrune"], ["--ldWindow"], ["--ldR2"], ["--ld", ""], ["--ldPrune="], ["--ldWindow", "0"],
                 ["--ldWindow", "513"], ["--ldWindow", "5x"], ["--ldWindow", "-1"], ["--ldR2", "1.1"], ["--ldR2", ".2"],
                 ["--ldR2", "2e-1"], ["--ldR2", "+0.2"], ["--ldR2", "0.3333333"], ["--ldR2", " 0.2"]):
        p = cli(args, vcf)
        assert p.returncode == 2 and p.stderr.count(b"\n") == 1 and p.stdout == b"", (args, p.stderr)
    for flag, path in (("--ld", tmp_path / "no_such_dir" / "x.ld"), ("--ldPrune", tmp_path / "no_such_dir" / "x")):
        p = cli([flag, str(path)], vcf)
        assert p.returncode == 1 and p.stderr.count(b"\n") == 1 and b"no_such_dir" in p.stderr, p.stderr


# ---- the golden 1KG slice

def test_golden_1kg(bv, golden_1kg, monkeypatch, tmp_path):
    """N = 50, --ldR2 0.2 against the numpy reference: the table and both lists byte for byte"""
    vcf = golden_1kg[0]
    want, out_o, log_o = lp.expected(orc.run, vcf, 50, 200000)
    assert want["bed"].shape[1] == 626 and len(want["events"]) > 1000
    for path in ("streaming", "census"):
        use_path(monkeypatch, path)
        rc, out, log, table, pin, pout = run_with_ld(bv, vcf, tmp_path, 50, "0.2", tag=path)
        assert rc == 0, log
        assert out == out_o and log == log_o
        same_files((table, pin, pout), want)
