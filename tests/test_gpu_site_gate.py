"""The site gate on the device (bvcf_sitegate.hip.h, bvcf_set_site_gate): the exact HWE test as k_site_gate / k_site_hwe run
it, against the references of sitegate.py, and whole runs with a gate against the oracle's run of the same bytes with the
failing rows taken out (sitegate.gate): the TSV, the log, the dosage rows, the --sampleStats and --relatedness tables and
the report.  tests/test_site_gate_cpu.py checks the inputs and thresholds used here with the oracle alone."""
import gzip
import hashlib
import os
import subprocess

import numpy as np
import pytest

import bgzf
import oracle_lib as orc
import pairtable as pt
import samplecut
import sitegate as sg
from test_gpu_sample_stats import table_from_tsv

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


def n_terms(t):
    return len(sg.support(*t)[2])


# ---- the exact test on the device

def check_p(bv, triples, ref=sg.hwe_ref):
    got = bv.bench_hwe(triples)
    worst = (0.0, ())
    for t, g in zip(triples, got):
        want = ref(*t)
        if want > sg.HWE_TINY:
            worst = max(worst, (abs(float(g) - want) / want, t))
        assert sg.close(float(g), want), (t, float(g), want)
    print("%d triples, worst relative error %.2e at %s" % (len(triples), worst[0], worst[1]))
    return got


def test_hwe_every_small_triple(bv):
    check_p(bv, sg.small_triples(12))


@pytest.mark.parametrize("n", sg.DEVICE_SIZES)
def test_hwe_seeded_triples(bv, n):
    """n = 63: every support has at most 32 terms, the thread's recurrence, with all-het at the bound; 64 and 65: all-het
    has 33, the first supports a wave sums; beyond: both kinds.  (tests/test_site_gate_cpu.py ties the lists to the bound
    the library exports and checks their term ratios against the tie factor.)"""
    tr = sg.device_triples(n)
    terms = [n_terms(t) for t in tr]
    bound = bv.hwe_inline_terms()
    assert min(terms) <= bound and (max(terms) > bound) == (n >= 64) and (n != 63 or max(terms) == bound)
    check_p(bv, tr)


def test_hwe_corners(bv):
    got = check_p(bv, sg.ALL_HET)
    assert sg.ALL_HET[-1] == (1000, 0, 0) and 0 < float(got[-1]) < 1e-200
    assert [float(x) for x in bv.bench_hwe(sg.ONE_TERM)] == [1.0] * len(sg.ONE_TERM)  # one term (or the only het possible)
    under = float(bv.bench_hwe([sg.UNDERFLOW])[0])
    assert under == under and 0.0 <= under < sg.HWE_TINY
    check_p(bv, sg.SEGMENTS)


# ---- whole runs

_ORACLE = {}


def oracle_side(vcf, cfg):
    key = (hashlib.sha256(vcf).digest(), tuple(sorted(cfg.items())))
    if key not in _ORACLE:
        rc, out, log, _ = orc.run(vcf, cfg)
        assert rc == 0
        _ORACLE[key] = (out, log)
    return _ORACLE[key]


_WANT = {}


def expected(bv, vcf, criteria, cfg):
    """what a gated run of `vcf` must produce, from the oracle's run of the same bytes: computed once, shared by the chains"""
    key = (hashlib.sha256(vcf).digest(), tuple(sorted(criteria.items())), tuple(sorted(cfg.items())))
    if key not in _WANT:
        out, log = oracle_side(vcf, cfg)
        names = pt.sample_names(vcf)
        mask, counts, report = sg.gate(out, len(names), criteria, cfg)
        body = sg.kept_body(out, mask)
        w = {"body": body, "log": log, "mask": mask, "counts": counts, "report": report}
        if names:
            w["stats"] = table_from_tsv(bv, body, names, cfg)
            w["pairs"] = pt.file_text(pt.tables(*pt.matrices(body, names, cfg)), names, cfg.get("emptyField", "!"))
        _WANT[key] = w
    return _WANT[key]


def first_diff(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (x, y) in enumerate(zip(g, w)):
        if x != y:
            return "line %d:\n got  %r\n want %r" % (i, x[:200], y[:200])
    return "lengths %d vs %d lines" % (len(g), len(w))


def check_run(bv, vcf, criteria, tmp_path, cfg=None, expect_of=None, pairs=True, **kw):
    """bvcf_run_buffer of the original bytes with the gate and every table; expect_of: the bytes the oracle runs (the
    masked or cut file of a composed case)"""
    cfg = dict(cfg or {})
    base = {k: v for k, v in cfg.items() if k not in ("minGQ", "minDP", "keepSamples", "excludeSamples")}
    w = expected(bv, vcf if expect_of is None else expect_of, criteria, base)
    files = {k: str(tmp_path / k) for k in ("sampleStats", "relatedness", "siteFilterReport")}
    if not pairs:
        del files["relatedness"]
    rc, out, log, _ = bv.run_buffer(vcf, dict(cfg, **criteria, **files), **kw)
    assert rc == 0, log
    assert out == w["body"], first_diff(out, w["body"])
    assert log == w["log"]
    got = {k: open(p, "rb").read() for k, p in files.items()}
    assert got["siteFilterReport"] == w["report"], (got["siteFilterReport"], w["report"])
    assert got["sampleStats"] == w["stats"], first_diff(got["sampleStats"], w["stats"])
    if pairs:
        assert got["relatedness"] == w["pairs"], first_diff(got["relatedness"], w["pairs"])
    return w


def split_file(vcf):
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


def oracle_dosage_kept(vcf, cfg, mask):
    """the oracle's --dosageOutput rows (main.go:576-584; one per TSV row, in its order) of the rows that stay:
    (loci, int8 matrix).  As oracle_lib.run_dosage, but only the kept rows are parsed"""
    import ctypes as C
    L = orc.lib()
    L.orc_run_dosage.argtypes = [C.POINTER(orc.OrcConfig), C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.orc_run_dosage.restype = C.c_int
    c = orc.make_config(cfg, 1)
    out, n_out = C.c_void_p(), C.c_size_t()
    rc = L.orc_run_dosage(C.byref(c), vcf, len(vcf), C.byref(out), C.byref(n_out))
    text = C.string_at(out, n_out.value)
    L.orc_free(out)
    assert rc == 0
    lines = text.split(b"\n")[:-1]
    assert len(lines) == len(mask)
    S = len(pt.sample_names(vcf))
    kept = [ln.partition(b"\t") for ln, k in zip(lines, mask) if k]
    m = np.zeros((len(kept), S), dtype=np.int8)
    for r, (_, _, d) in enumerate(kept):
        one = d.replace(b"-1", b"/")  # ("/" is "0" - 1: single-character values are read without a text parser)
        if len(one) == 2 * S - 1:
            m[r] = np.frombuffer(one, dtype=np.uint8)[::2].astype(np.int16) - 48
        else:
            m[r] = [int(x) for x in d.split(b",")]
    m.setflags(write=False)
    return [locus.decode() for locus, _, _ in kept], m


def check_records(bv, vcf, criteria, cfg=None, expect_of=None, pairs=False, **ctx_kw):
    """the file's blocks through a ctx with the gate (ctx_kw: min_gq / sample_keep of a composed case; expect_of: the masked
    or cut bytes the oracle runs): every examined record against sitegate.verdict, the batches' counts, the dosage rows of
    the rows that stay against the oracle's, and with pairs the bvcf_pair_stats tables against pairtable.tables over
    the kept rows"""
    cfg = cfg or {}
    ref = vcf if expect_of is None else expect_of
    w = expected(bv, ref, criteria, cfg)
    out, _ = oracle_side(ref, cfg)
    names = pt.sample_names(ref)
    S = len(names)
    rows = [sg.row_counts(r.split(b"\t"), cfg) for r in out.split(b"\n") if r]
    if "dosage" not in w:
        w["dosage"] = oracle_dosage_kept(ref, cfg, w["mask"])[1]
    if pairs and "tables" not in w:
        w["tables"] = pt.tables(*pt.matrices(w["body"], names, cfg))
        w["tables"].setflags(write=False)
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, allow=cfg.get("allow", "PASS,."), eol_chars=eol, want_dosage=True, site_gate=criteria, pair_stats=pairs,
                 **ctx_kw)
    counts = [0] * 7
    examined, dosage = [], []
    for blk in blocks_of(data):
        b = ctx.process(blk)
        counts = [x + y for x, y in zip(counts, b.gate_counts)]
        kept_slots = []
        for i in range(b.n_lines):
            if int(b.lines[i]["status"]) != bv.LINE_OK:
                continue
            for k in b.record_slots(i):
                A = b.alleles[k]
                bits = int(A["pad"][0])
                if int(A["ac"]) == 0 and bits == 0:
                    continue  # a row no sample carries: not examined
                assert (int(A["ac"]) == 0) == (bits != 0), "a gated record has ac == 0 and a non-zero gate byte"
                examined.append((bits, int(A["an"]), int(A["n_het"]), int(A["n_hom"]), int(A["n_miss"])))
                if bits == 0:
                    kept_slots.append(k)
        dosage.append(np.array(b.dosage[np.array(kept_slots, dtype=np.int64), :S], dtype=np.int8).reshape(len(kept_slots), S))
    got_tables = ctx.pair_stats() if pairs else None
    ctx.close()
    assert counts == w["counts"], (counts, w["counts"])
    assert len(examined) == len(rows)
    for got, c in zip(examined, rows):
        assert got == (sg.verdict(criteria, S, c),) + c[1:], (got, c)  # the fail bits; an .. n_miss stay as they were
    dosage = np.concatenate(dosage)
    assert dosage.shape == w["dosage"].shape
    bad = np.argwhere(dosage != w["dosage"])
    assert not len(bad), "dosage: %d cells differ, first at kept row %d sample %d" % (len(bad), bad[0][0], bad[0][1])
    if pairs:
        assert got_tables.shape == w["tables"].shape and np.array_equal(got_tables, w["tables"])


@pytest.mark.parametrize("name", ["rare63", "rare64", "rare65", "rare300", "short", "sweep", "fuzz13"])
def test_chains_and_map_forms(bv, chain, tmp_path, name):
    """both chains and the streaming kernel for GT:DP:GQ fields (fuzz13); short class lists and dense maps"""
    check_run(bv, sg.case_input(name), sg.CASES[name][0], tmp_path)
    check_records(bv, sg.case_input(name), sg.CASES[name][0])


@pytest.mark.parametrize("name,k", [(n, k) for n in ("rare300", "sweep", "short") for k in range(1, len(sg.CASES[n]))])
def test_each_criterion_alone(bv, chain, tmp_path, name, k):
    check_run(bv, sg.case_input(name), sg.CASES[name][k], tmp_path)


@pytest.mark.parametrize("name,k", [(n, k) for n in ("tile1", "tile63", "tile64", "tile65", "tile130") for k in range(len(sg.CASES[n]))])
def test_row_counts_at_the_wave_edges(bv, chain, tmp_path, name, k):
    w = check_run(bv, sg.case_input(name), sg.CASES[name][k], tmp_path)
    assert w["counts"][0] == int(name[4:])
    check_records(bv, sg.case_input(name), sg.CASES[name][k])


@pytest.mark.parametrize("k", [0, 1])
def test_one_sample(bv, chain, tmp_path, k):
    w = check_run(bv, sg.case_input("one"), sg.CASES["one"][k], tmp_path)
    assert 0 < w["counts"][1] < w["counts"][0]
    check_records(bv, sg.case_input("one"), sg.CASES["one"][k], pairs=True)


def test_neutral_gate_changes_nothing(bv, chain, tmp_path):
    vcf = sg.case_input("sweep")
    w = check_run(bv, vcf, dict(sg.NEUTRAL), tmp_path)
    out, log = oracle_side(vcf, {})
    assert w["body"] == out and w["counts"][0] == w["counts"][1] == out.count(b"\n") and not any(w["counts"][2:])
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, site_gate=dict(sg.NEUTRAL))
    b = ctx.process(data)
    ctx.close()
    assert not b.alleles["pad"][:, 0].any()


def test_composed_with_min_gq(bv, tmp_path):
    """--minGQ masks first: the gate sees the masked counts"""
    check_run(bv, sg.case_input("fuzz13"), sg.MASKED13, tmp_path, {"minGQ": sg.MASK_GQ}, expect_of=sg.case_input("masked13"))
    check_records(bv, sg.case_input("fuzz13"), sg.MASKED13, expect_of=sg.case_input("masked13"), pairs=True, min_gq=sg.MASK_GQ)


def test_composed_with_keep_samples(bv, tmp_path):
    """--keepSamples cuts first: S and every count are those of the kept samples"""
    vcf = sg.case_input("rare300")
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], sg.CUT_KEEP)
    check_run(bv, vcf, sg.WIDE, tmp_path, {"keepSamples": lst}, expect_of=sg.case_input("cut300"))
    check_records(bv, vcf, sg.WIDE, expect_of=sg.case_input("cut300"), pairs=True, sample_keep=sg.CUT_KEEP)


def test_golden_1kg(bv, golden_1kg, chain, tmp_path):
    """2 504 samples, supports of up to 1 253 terms, 40 x 40 pair blocks.  The --relatedness file of 2 504 samples has
    3.1 M lines: the run writes the TSV, the --sampleStats table and the report, and the gated pair counts are compared as
    the ctx's bvcf_pair_stats tables -- what the file is derived from -- with the records and the dosage rows"""
    w = check_run(bv, golden_1kg[0], sg.GOLDEN, tmp_path, pairs=False)
    assert w["counts"][0] == 19821 and 1000 < w["counts"][1] < 19821
    check_records(bv, golden_1kg[0], sg.GOLDEN, pairs=True, want_class_maps=False)
    assert w["tables"].shape == (3, 2504, 2504) and w["dosage"].shape == (w["counts"][1], 2504)


def test_set_site_gate_on_a_ctx(bv):
    for bad in ({"minMaf": 0.6}, {"hwe": float("nan")}, {"maxMissing": 1.5}):
        with pytest.raises(bv.BvcfError) as ei:
            bv.Ctx(9 + 4, site_gate=bad)
        assert ei.value.rc == bv.E_ARG
    ctx = bv.Ctx(9, site_gate=sg.RARE)  # no sample columns: a no-op
    b = ctx.process(b"chr1\t100\t.\tA\tC\t50\tPASS\t.\n")
    assert b.gate_counts == [0] * 7
    ctx.close()


# ---- the CLI (each run under its own time limit)

def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


@pytest.fixture(scope="module")
def cohort(bv, tmp_path_factory):
    d = tmp_path_factory.mktemp("sg")
    vcf = sg.case_input("cohort")
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    return vcf, paths, d, expected(bv, vcf, sg.COHORT, {})


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, w = cohort
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        rep, st, pr = (d / ("%s.%s" % (tag, x)) for x in ("report", "stats", "pairs"))
        p = cli(args + sg.cli_args(sg.COHORT, rep) + ["--sampleStats", str(st), "--relatedness", str(pr)], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == w["body"], (tag, first_diff(p.stdout.split(b"\n", 1)[1], w["body"]))
        assert p.stderr.decode() == w["log"], tag
        assert rep.read_bytes() == w["report"], (tag, rep.read_bytes())
        assert st.read_bytes() == w["stats"], tag
        assert pr.read_bytes() == w["pairs"], tag


def read_matrix(path):
    import pyarrow.ipc as ipc
    t = ipc.open_file(str(path)).read_all()
    m = np.stack([t.column(i).to_numpy() for i in range(1, t.num_columns)], axis=1).astype(np.int8)
    return t.column(0).to_pylist(), m


def test_cli_bgzf_output_and_dosage_file_follow_the_gate(bv, cohort):
    """the dosage file holds the oracle's rows of the rows that stay, loci and order included; --compressOutput bgzf
    changes neither it nor the TSV's text; --noOut with a dosage file alone gives the same file"""
    pytest.importorskip("pyarrow")
    vcf, paths, d, w = cohort
    loci, want = oracle_dosage_kept(vcf, {}, w["mask"])
    outs = {}
    for tag, extra in (("plain", []), ("bgzf", ["--compressOutput", "bgzf"])):
        tsv, dos = d / ("o.%s.tsv" % tag), d / ("o.%s.arrow" % tag)
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--dosageOutput", str(dos)] + sg.cli_args(sg.COHORT) + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        outs[tag] = (tsv.read_bytes(), dos)
    assert outs["plain"][0].split(b"\n", 1)[1] == w["body"]
    assert gzip.decompress(outs["bgzf"][0]) == outs["plain"][0]
    nout = d / "o.noout.arrow"
    p = cli(["--in", str(paths["text"]), "--noOut", "--batchMB", "1", "--dosageOutput", str(nout)] + sg.cli_args(sg.COHORT))
    assert p.returncode == 0 and p.stdout == b"", p.stderr[-400:]
    for dos in (outs["plain"][1], outs["bgzf"][1], nout):
        got_loci, got = read_matrix(dos)
        assert got_loci == loci and got.shape == want.shape and np.array_equal(got, want), str(dos)


def test_cli_no_out_report_alone_is_a_qc_pass(bv, cohort):
    vcf, paths, d, w = cohort
    rep = d / "noout.report"
    p = cli(["--in", str(paths["text"]), "--noOut"] + sg.cli_args(sg.COHORT, rep))
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == b"" and rep.read_bytes() == w["report"]
    p = cli(["--in", str(paths["text"]), "--noOut"] + sg.cli_args(sg.COHORT))  # thresholds alone make no output
    assert p.returncode == 1 and b"When specifying --noOut, must specify --dosageOutput" in p.stderr


def test_cli_sites_only_and_unwritable(bv, tmp_path):
    import vcfgen
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    plain = cli([], vcf)
    rep = tmp_path / "sites.report"
    p = cli(sg.cli_args(sg.RARE, rep), vcf)
    assert p.returncode == 0 and plain.returncode == 0, p.stderr[-400:]
    assert p.stdout == plain.stdout and p.stderr == plain.stderr  # nothing is examined: unchanged
    assert rep.read_bytes() == sg.report_text([0] * 7)
    bad = tmp_path / "no_such_dir" / "x.report"
    p = cli(sg.cli_args(sg.RARE, bad), vcf)
    assert p.returncode == 1 and str(bad).encode() in p.stderr and p.stdout == b""
