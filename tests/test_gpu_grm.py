"""--grm: the GRM's integer tables made on the device (bvcf_grm.hip.h, bvcf_enable_grm, bvcf_grm) and the three files
written from them.

The expected tables and bytes come from the oracle's TSV of the same bytes (grm.py): dosage matrices of the rows'
heterozygotes / homozygotes / missingGenos lists, quantised by the definition in Python integers and multiplied exactly.
Every comparison is byte for byte (the files) or integer for integer (the tables): there is no tolerance."""
import gzip
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf
import grm
import gtmask
import oracle_lib as orc
import pairtable as pt
import regions as rg
import samplecut
import sitegate as sg
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")
SUFFIXES = (".grm.bin", ".grm.N.bin", ".grm.id")
MAX_LINES = 60000  # (a ctx with the GRM on reserves at most GRM_MAX_BATCH_ROWS allele slots: 2 * max_lines + 1024)


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
    """every device path that leaves class maps (as in test_gpu_pair_stats.py)"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.fixture(params=["census", "streaming"])
def two_paths(request, monkeypatch):
    """dense maps only, and both map forms"""
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def split_file(vcf):
    """-> (header fields, eol_chars, the data lines' bytes)"""
    at = vcf.index(b"#CHROM")
    end = vcf.index(b"\n", at)
    crlf = vcf[end - 1:end] == b"\r"
    return len(vcf[at:end - crlf].split(b"\t")), 2 if crlf else 1, vcf[end + 1:]


def signed(lo, hi):
    """bvcf_grm's words of T as int64 (every test's sums fit; the high word is then the sign's extension)"""
    t = lo.view(np.int64)
    assert np.array_equal(hi, (t >> 63).view(np.uint64)), "T left 64 bits"
    return t


def ctx_tables(bv, vcf, allow="PASS,.", block_lines=None, **kw):
    """(T int64, MM int64, N) of a ctx that the file's data lines went through"""
    nh, eol, data = split_file(vcf)
    kw.setdefault("max_lines", MAX_LINES)
    ctx = bv.Ctx(nh, allow=allow, eol_chars=eol, grm=True, **kw)
    try:
        if block_lines is None:
            ctx.process(data)
        else:
            lines = data.split(b"\n")[:-1]
            for i in range(0, len(lines), block_lines):
                ctx.process(b"".join(x + b"\n" for x in lines[i:i + block_lines]))
        lo, hi, mm, n = ctx.grm_words()
        return signed(lo, hi), mm.astype(np.int64), n
    finally:
        ctx.close()


def read_files(prefix):
    out = []
    for sfx in SUFFIXES:
        with open(str(prefix) + sfx, "rb") as f:
            out.append(f.read())
    return tuple(out)


def run_with_grm(bv, vcf, tmp_path, cfg=None, **kw):
    """bvcf_run_buffer with --grm -> (rc, TSV body, log, the three files' bytes)"""
    prefix = str(tmp_path / "m")
    c = dict(cfg or {})
    c["grm"] = prefix
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    return rc, out, log, read_files(prefix)


def tables_diff(got, want):
    for name, g, w in zip(("T", "MM"), got[:2], want[:2]):
        if g.shape != w.shape:
            return "%s: shape %s, want %s" % (name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        if len(bad):
            i, j = (int(x) for x in bad[0])
            return "%s: %d elements differ; first [%d][%d]: got %d want %d" % (name, len(bad), i, j, g[i, j], w[i, j])
    return "N: got %d want %d" % (got[2], want[2])


def same_tables(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def files_diff(got, want):
    for sfx, g, w in zip(SUFFIXES, got, want):
        if g != w:
            if len(g) != len(w):
                return "%s: %d bytes, want %d" % (sfx, len(g), len(w))
            if sfx == ".grm.id":
                return "%s differs" % sfx
            a, b = np.frombuffer(g, "<f4"), np.frombuffer(w, "<f4")
            k = int(np.argwhere(a.view(np.uint32) != b.view(np.uint32))[0][0])
            return "%s: float %d: got %r want %r" % (sfx, k, float(a[k]), float(b[k]))
    return "equal"


_WANT = {}


def oracle_side(vcf, cfg=None):
    """((T, MM, N), the three files' bytes, TSV body, log) from the oracle: computed once per input and config, shared by
    the device paths"""
    cfg = cfg or {}
    key = (hashlib.sha256(vcf).digest(), tuple(sorted(cfg.items())))
    if key not in _WANT:
        t, files, body, log = grm.expected(orc.run, vcf, cfg)
        for x in t[:2]:
            x.setflags(write=False)
        _WANT[key] = (t, files, body, log)
    return _WANT[key]


def check_both(bv, vcf, tmp_path, cfg=None):
    """raw tables through a ctx and the files through bvcf_run_buffer, against the oracle's"""
    cfg = cfg or {}
    want_t, want_files, out_o, log_o = oracle_side(vcf, cfg)
    rc, out, log, files = run_with_grm(bv, vcf, tmp_path, cfg)
    assert rc == 0, log
    assert out == out_o and log == log_o, "the TSV / log changed with --grm"
    got_t = ctx_tables(bv, vcf, allow=cfg.get("allow", "PASS,."))
    assert same_tables(got_t, want_t), tables_diff(got_t, want_t)
    assert files == want_files, files_diff(files, want_files)
    return want_t


# ---- table cases

@pytest.mark.parametrize("seed", [s[0] for s in pt.FUZZ])
def test_fuzz(bv, bvcf_path, tmp_path, seed):
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",",
                                          "emptyField": "NA"}
    check_both(bv, pt.fuzz_vcf(seed), tmp_path, cfg)


@pytest.mark.parametrize("ns", grm.SAMPLE_EDGES)
def test_sample_edges(bv, two_paths, tmp_path, ns):
    """1 .. 300 samples: an MFMA block short of, at and past 16 samples, a workgroup's block likewise at 64, five blocks at 300
    -- there i-block != j-block with different samples on either side, so a transposed C/D write cannot pass"""
    T, MM, N = check_both(bv, grm.edge_vcf(ns), tmp_path)
    if ns == 300:
        assert not np.array_equal(T[:64, 64:128], T[:64, 64:128].T)


def test_both_map_forms_are_reached(bv, monkeypatch):
    """the streaming path keeps rare alleles as short class lists and common ones as dense maps: k_grm_gemm and
    k_grm_sparse both add there"""
    monkeypatch.setenv("BVCF_PATH", "2")
    nh, eol, data = split_file(pt.rare_vcf(300))
    ctx = bv.Ctx(nh, grm=True, max_lines=MAX_LINES)
    b = ctx.process(data)
    forms = {"sparse": 0, "dense": 0}
    for i in range(b.n_lines):
        if int(b.lines[i]["status"]) != bv.LINE_OK:
            continue
        for slot in b.record_slots(i):
            A = b.alleles[slot]
            if int(A["ac"]) and int(A["cmap_off"]) != bv.NO_CMAP:
                forms["sparse" if int(A["flags"]) & 2 else "dense"] += 1
    ctx.close()
    assert forms["sparse"] > 50 and forms["dense"] > 20, forms


def test_rare_carriers(bv, bvcf_path, tmp_path):
    check_both(bv, pt.rare_vcf(300), tmp_path)


@pytest.mark.parametrize("n_rows", pt.TILE_ROWS)
def test_row_tile_edges(bv, monkeypatch, tmp_path, n_rows):
    """1, 63, 64, 65 and 130 dense rows: a k-step short of, at and past its 64 rows"""
    for k, v in PATHS["census"].items():
        monkeypatch.setenv(k, v)
    check_both(bv, pt.tile_vcf(n_rows), tmp_path)


def test_short_list_at_its_limit(bv, bvcf_path, tmp_path):
    """15 entries x 4 samples, missing calls among them"""
    check_both(bv, pt.short_list_limit_vcf(), tmp_path)


def test_half_missing_and_all_missing_samples(bv, bvcf_path, tmp_path):
    check_both(bv, pt.half_missing_vcf(), tmp_path)
    T, MM, N = check_both(bv, grm.all_missing_sample_vcf(), tmp_path)
    assert N > 0 and int(MM[2, 2]) == N  # sample 2 is never called: N(i,2) = 0 and A(i,2) = 0 in the file


def test_all_het_rows_count_and_all_hom_rows_do_not(bv, bvcf_path, tmp_path):
    vcf = grm.monomorphic_vcf()
    T, MM, N = check_both(bv, vcf, tmp_path)
    assert 0 < N < orc.run(vcf)[1].count(b"\n")


def test_singleton_hom_three_limbs(bv, two_paths, tmp_path):
    check_both(bv, grm.singleton_hom_vcf(), tmp_path)


def test_int32_sums_are_flushed(bv, monkeypatch):
    """150 000 identical dense rows in ONE batch: the low-limb products of one pair add up past 2^31"""
    for k, v in PATHS["census"].items():
        monkeypatch.setenv(k, v)
    gts, v = grm.flush_pattern()
    assert v * grm.FLUSH_ROWS >= 1 << 31
    one = (vcfgen.header(8) + pt.snp_line(100, gts)).encode()
    (T1, MM1, N1), _, _, _ = oracle_side(one)
    assert N1 == 1
    got = ctx_tables(bv, grm.flush_vcf(), max_batch_bytes=16 << 20, max_lines=grm.FLUSH_ROWS + 100, max_alleles=grm.FLUSH_ROWS + 200)
    want = (T1 * grm.FLUSH_ROWS, MM1 * grm.FLUSH_ROWS, grm.FLUSH_ROWS)
    assert same_tables(got, want), tables_diff(got, want)


def test_min_gq_masked_calls_are_missing(bv, bvcf_path, tmp_path):
    vcf = pt.fuzz_vcf(13)  # GT:DP:GQ, CRLF
    masked = gtmask.mask_vcf(vcf, 20, 0)
    want_t, want_files = oracle_side(masked)[:2]
    assert int(np.trace(want_t[1])) > int(np.trace(oracle_side(vcf)[0][1]))  # more missing calls
    rc, out, log, files = run_with_grm(bv, vcf, tmp_path, {"minGQ": 20})
    assert rc == 0, log
    assert files == want_files, files_diff(files, want_files)


def test_poisoned_allocations(bv, monkeypatch, tmp_path):
    """BVCF_POISON: every fresh buffer filled with 0xa5 and held between guards -- nothing is read before it is written,
    nothing written outside its buffer"""
    monkeypatch.setenv("BVCF_POISON", "a5")
    for k, v in PATHS["streaming"].items():
        monkeypatch.setenv(k, v)
    bv.guard_check()
    check_both(bv, pt.rare_vcf(300), tmp_path)
    n, msg = bv.guard_check()
    assert n == 0, "%d buffer(s) written out of bounds, the first: %s" % (n, msg)


# ---- the 1KG slice: 2 504 samples, 40 x 40 pair blocks

@pytest.fixture(scope="module")
def golden(golden_1kg):
    """the slice's TSV body and dosage matrices through the oracle, once"""
    vcf = golden_1kg[0]
    rc, body, _, _ = orc.run(vcf)
    assert rc == 0
    names = pt.sample_names(vcf)
    H, O, M = pt.matrices(body, names)
    for x in (H, O, M):
        x.setflags(write=False)
    return vcf, body, names, (H, O, M)


def golden_files(golden, mask=None, cols=None):
    """the three files of the slice's rows that stay (mask) over the samples that stay (cols; a row no kept sample carries is
    no row)"""
    vcf, body, names, (H, O, M) = golden
    if mask is not None:
        keep = np.asarray(mask, dtype=bool)
        H, O, M = H[keep], O[keep], M[keep]
    if cols is not None:
        H, O, M = H[:, cols], O[:, cols], M[:, cols]
        rows = (H.sum(axis=1) + O.sum(axis=1)) > 0
        H, O, M = H[rows], O[rows], M[rows]
        names = [names[c] for c in cols]
    t = grm.tables(H, O, M)
    return t, grm.files(*t, names)


@pytest.fixture(scope="module")
def golden_full(golden):
    return golden_files(golden)


def cli(args, stdin_bytes=None, timeout=300, env=None):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout, env=env)


def test_golden_many_batches_and_a_reset(bv, golden, golden_full, monkeypatch):
    """the slice in batches of 1 500 lines, two in flight, maps made on the device only; the totals are read and reset half
    way: the two readings add up to the whole"""
    monkeypatch.setenv("BVCF_PATH", "2")
    vcf = golden[0]
    nh, eol, data = split_file(vcf)
    lines = data.split(b"\n")[:-1]
    blocks = [b"".join(x + b"\n" for x in lines[i:i + 1500]) for i in range(0, len(lines), 1500)]
    assert len(blocks) > 10
    ctx = bv.Ctx(nh, n_slots=2, grm=True, want_class_maps=False, max_batch_bytes=32 << 20, max_lines=4000)
    pending = 0
    first = None
    for k, blk in enumerate(blocks):
        ctx.submit(blk, k)
        pending += 1
        if pending == 2:
            ctx.collect()
            pending -= 1
        if k == len(blocks) // 2:
            first = ctx.grm_words(reset=True)
    while pending:
        ctx.collect()
        pending -= 1
    second = ctx.grm_words(reset=True)
    assert not any(x.any() for x in ctx.grm_words()[:3]) and ctx.grm_words()[3] == 0
    ctx.close()
    assert first[3] > 0 and second[3] > 0
    got = (signed(first[0], first[1]) + signed(second[0], second[1]), (first[2] + second[2]).astype(np.int64), first[3] + second[3])
    want = golden_full[0]
    assert same_tables(got, want), tables_diff(got, want)


def test_golden_cli_min_gq_runs_the_masked_scan(bv, golden_full, tmp_path):
    """the slice has no GQ: --minGQ masks nothing, and the files are the plain ones -- through the census chain's masked scan"""
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--minGQ", "20", "--grm", str(tmp_path / "g")])
    assert p.returncode == 0, p.stderr[-400:]
    got = read_files(tmp_path / "g")
    assert got == golden_full[1], files_diff(got, golden_full[1])


def test_golden_cli_keep_samples(bv, golden, tmp_path):
    """200 kept samples, in rank space: the rows no kept sample carries are no rows, n and a are over the kept samples"""
    vcf = golden[0]
    idx = sorted(random.Random(77).sample(range(2504), 200))
    want = golden_files(golden, cols=idx)[1]
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx)
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--keepSamples", lst, "--grm", str(tmp_path / "g")])
    assert p.returncode == 0, p.stderr[-400:]
    got = read_files(tmp_path / "g")
    assert len(got[0]) == 4 * 200 * 201 // 2
    assert got == want, files_diff(got, want)


def test_golden_cli_min_maf_survivors(bv, golden, tmp_path):
    """--minMaf 0.01: the GRM over the rows the site gate leaves"""
    vcf, body, names, _ = golden
    mask = sg.gate(body, len(names), {"minMaf": 0.01})[0]
    assert 1000 < sum(mask) < len(mask) - 1000
    want = golden_files(golden, mask=mask)[1]
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--minMaf", "0.01", "--grm", str(tmp_path / "g")])
    assert p.returncode == 0, p.stderr[-400:]
    got = read_files(tmp_path / "g")
    assert got == want, files_diff(got, want)


def test_golden_cli_regions(bv, golden, tmp_path):
    """--regions: the GRM over the middle third of the slice"""
    vcf, body, names, _ = golden
    sets = rg.golden_sets(body)[0]
    mask = rg.select(body, sets)
    assert 1000 < sum(mask) < len(mask) - 1000
    want = golden_files(golden, mask=mask)[1]
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--grm", str(tmp_path / "g")] + sets.cli_args(tmp_path))
    assert p.returncode == 0, p.stderr[-400:]
    got = read_files(tmp_path / "g")
    assert got == want, files_diff(got, want)


# ---- the Ctx

def test_ctx_that_was_not_enabled(bv):
    ctx = bv.Ctx(9 + 4)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.grm_words()
    assert ei.value.rc == bv.E_ARG
    ctx.close()


def test_ctx_above_the_caps(bv):
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9 + bv.PAIR_MAX_SAMPLES + 1, grm=True, max_batch_bytes=1 << 20, max_lines=1000)
    assert ei.value.rc == bv.E_ARG and "8192" in str(ei.value)
    with pytest.raises(bv.BvcfError) as ei:  # more allele slots than a batch's int64 tables hold rows
        bv.Ctx(9 + 4, grm=True, max_lines=bv.GRM_MAX_BATCH_ROWS)
    assert ei.value.rc == bv.E_TOO_BIG and str(bv.GRM_MAX_BATCH_ROWS) in str(ei.value)
    ctx = bv.Ctx(9, grm=True)  # no sample columns: a no-op, and an empty table
    lo, hi, mm, n = ctx.grm_words()
    assert lo.shape == (0, 0) and n == 0
    ctx.close()


# ---- the CLI (each run under its own time limit)

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("grm")
    vcf = vcfgen.gen_vcf(41, 3000, 400, weird=0.02) + vcfgen.gen_vcf(42, 1500, 400, weird=0.02).split(b"\n", 3)[3]
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    t, files, out_o, _ = grm.expected(orc.run, vcf)
    return vcf, paths, d, out_o, files


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        p = cli(args + ["--grm", str(d / tag)], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        got = read_files(d / tag)
        assert got == want, (tag, files_diff(got, want))


def test_cli_no_out_grm_only_pass(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    p = cli(["--in", str(paths["text"]), "--noOut", "--grm", str(d / "noout")])
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == b""
    assert read_files(d / "noout") == want


def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d, out_o, want = cohort
    outs = {}
    for tag, extra in (("plain", []), ("grm", ["--grm", str(d / "o")])):
        tsv, dos, smp, sst, prs = (d / ("%s.%s" % (tag, x)) for x in ("tsv.gz", "arrow", "samples", "stats", "pairs"))
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--compressOutput", "bgzf", "--dosageOutput", str(dos),
                 "--sample", str(smp), "--sampleStats", str(sst), "--relatedness", str(prs), "--plinkOutput", str(d / tag)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        made = [tsv, dos, smp, sst, prs] + [d / (tag + x) for x in (".bed", ".bim", ".fam")]
        outs[tag] = tuple(hashlib.sha256(f.read_bytes()).hexdigest() for f in made) + (p.stderr,)
    assert outs["plain"] == outs["grm"]
    assert read_files(d / "o") == want


def test_cli_exit_codes(bv, tmp_path):
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    # a file without sample columns: three empty files
    p = cli(["--grm", str(tmp_path / "sites")], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    assert read_files(tmp_path / "sites") == (b"", b"", b"")
    # an unwritable path: one message, nothing on stdout
    bad = tmp_path / "no_such_dir" / "x"
    p = cli(["--grm", str(bad)], vcf)
    assert p.returncode == 1 and str(bad).encode() in p.stderr and p.stderr.count(b"\n") == 1
    assert p.stdout == b""
    # the flag without a value
    p = cli(["--grm"], vcf)
    assert p.returncode == 2
    # one sample too many: one message, before anything is allocated
    ns = 8193
    wide = (vcfgen.header(ns) + "\t".join(["chr1", "100", ".", "A", "C", "50", "PASS", ".", "GT"] + ["0|1"] * ns) + "\n").encode()
    p = cli(["--grm", str(tmp_path / "wide")], wide)
    assert p.returncode == 1
    assert p.stderr.count(b"\n") == 1 and b"8193 samples" in p.stderr and b"8192" in p.stderr, p.stderr[-400:]
    assert read_files(tmp_path / "wide") == (b"", b"", b"")  # (opened early, written only by a run that succeeds)
