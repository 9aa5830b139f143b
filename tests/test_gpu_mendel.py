"""--mendel / --mendelErrors: the per-trio counts and the events made on the device (bvcf_mendel.hip.h, bvcf_enable_trios,
bvcf_trio_stats) and the two files written from them.

The expected table and list come from the oracle's TSV of the same bytes (mendel.py); both files must be equal byte for
byte, the per-batch table and events equal through a ctx, and the TSV and the log must be the oracle's."""
import gzip
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf
import gtmask
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


def oracle_side(vcf, fam, cfg=None):
    """(expected dict, TSV body, log) from the oracle: computed once per input, pedigree and config"""
    cfg = cfg or {}
    key = (hashlib.sha256(vcf).digest(), hashlib.sha256(fam).digest(), tuple(sorted(cfg.items())))
    if key not in _WANT:
        _WANT[key] = md.expected(orc.run, vcf, fam, cfg)
    return _WANT[key]


def run_with_mendel(bv, vcf, fam, tmp_path, cfg=None, tag="m", **kw):
    """bvcf_run_buffer with --fam / --mendel / --mendelErrors -> (rc, TSV body, log, --mendel bytes, --mendelErrors bytes)"""
    f = tmp_path / (tag + ".fam")
    f.write_bytes(fam)
    c = dict(cfg or {})
    c.update(fam=str(f), mendel=str(tmp_path / (tag + ".mendel")), mendelErrors=str(tmp_path / (tag + ".errors")))
    rc, out, log, _ = bv.run_buffer(vcf, c, **kw)
    return rc, out, log, (tmp_path / (tag + ".mendel")).read_bytes(), (tmp_path / (tag + ".errors")).read_bytes()


def first_diff(g, w):
    n = min(len(g), len(w))
    at = next((i for i in range(n) if g[i] != w[i]), n)
    return "%d vs %d bytes, first difference at byte %d: got %r want %r" % (len(g), len(w), at, g[at:at + 40], w[at:at + 40])


def check(bv, vcf, fam, tmp_path, cfg=None, **kw):
    want, out_o, log_o = oracle_side(vcf, fam, cfg)
    rc, out, log, mendel, errors = run_with_mendel(bv, vcf, fam, tmp_path, cfg, **kw)
    assert rc == 0, log
    assert out == out_o and log == log_o, "the TSV / log differ from the oracle's"
    assert mendel == want["mendel"], "--mendel: " + first_diff(mendel, want["mendel"])
    assert errors == want["errors"], "--mendelErrors: " + first_diff(errors, want["errors"])
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


def ctx_check(bv, vcf, want, **kw):
    """the whole file as one batch through a ctx: the batch's table and events -> the rows' forms"""
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, eol_chars=eol, trios=want["trios"], **kw)
    b = ctx.process(data)
    counts, events = ctx.trio_stats()
    info = ctx.trio_info()
    forms = row_forms(bv, b)
    ctx.close()
    assert info.n_trios == len(want["trios"]) and info.n_events == info.need_events == len(want["events"])
    assert np.array_equal(counts.astype(np.uint64), want["counts"]), "the batch's table differs"
    assert np.array_equal(events, want["events"]), "the batch's events differ"
    assert len(forms) == want["verdicts"].shape[0]
    return forms


def ped(vcf, trios):
    return md.fam_of(trios, pt.sample_names(vcf))


# ---- device paths

@pytest.mark.parametrize("seed", [11, 12, 14])
def test_fuzz(bv, bvcf_path, tmp_path, seed):
    vcf, fam = md.fuzz_inputs()["fuzz%d" % seed]
    cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",",
                                          "emptyField": "NA"}
    want = check(bv, vcf, fam, tmp_path, cfg)
    assert len(want["events"]) > 10 and len(want["trios"]) >= 5


def test_pedigree_both_map_forms(bv, bvcf_path, tmp_path):
    """300 samples, 90 trios (two chunks), short-list rows among dense rows: on the streaming path the batch held an event
    on a short-list row and one on a dense row"""
    vcf, trios = md.pedigree_vcf(300, 90, 120, 9800)
    want = check(bv, vcf, ped(vcf, trios), tmp_path)
    forms = np.array(ctx_check(bv, vcf, want))
    if bvcf_path == "streaming":
        ev_rows = np.zeros(len(forms), dtype=bool)
        ev_rows[want["events"][:, 0]] = True
        assert (ev_rows & forms).any() and (ev_rows & ~forms).any()


def test_all_27_informative_triples(bv, bvcf_path, tmp_path):
    vcf, trios = md.triples_vcf()
    want = check(bv, vcf, ped(vcf, trios), tmp_path)
    ctx_check(bv, vcf, want)
    # every trio sees all 27 triples: 12 inconsistent ones, of which 2 de novo -- but for the first, whose father is missing
    # in every fourth row
    assert (want["counts"][1:] == [27, 12, 2]).all() and want["counts"][0, 0] < 27


@pytest.mark.parametrize("n_trios", md.CHUNK_TRIOS)
def test_trio_chunk_edges(bv, monkeypatch, tmp_path, n_trios):
    """T = 1, 63, 64, 65, 130 with S = 3 T + 1: no, one full, one full and one, three chunks; S % 4 = 0, 2, 1, 0, 3"""
    vcf, trios = md.chunk_vcf(n_trios)
    assert len(pt.sample_names(vcf)) == 3 * n_trios + 1
    for path in ("streaming", "census"):
        use_path(monkeypatch, path)
        want = check(bv, vcf, ped(vcf, trios), tmp_path)
        ctx_check(bv, vcf, want)
        assert len(want["trios"]) == n_trios and (n_trios == 1 or len(want["events"]) > 0)


@pytest.mark.parametrize("n_rows", md.TILE_ROWS)
def test_row_tile_edges(bv, monkeypatch, tmp_path, n_rows):
    vcf, trios = md.tile_vcf(n_rows)
    for path in ("streaming", "census"):
        use_path(monkeypatch, path)
        want = check(bv, vcf, ped(vcf, trios), tmp_path)
        ctx_check(bv, vcf, want)
        assert want["verdicts"].shape == (n_rows, 23)


def test_short_list_at_its_limit(bv, monkeypatch, tmp_path):
    """lists of 15 entries and a row of 16 non-zero map bytes, under a random pedigree of 100 trios"""
    use_path(monkeypatch, "streaming")
    vcf = pt.short_list_limit_vcf(300)
    trios = md.random_trios(300, 100, 9810)
    want = check(bv, vcf, ped(vcf, trios), tmp_path)
    forms = ctx_check(bv, vcf, want)
    assert forms[:4] == [True, False, True, True], forms[:4]
    ev_rows = set(want["events"][:, 0].tolist())
    assert {0, 1, 2} <= ev_rows  # (60 carriers among 100 random trios: the full lists and the dense row hold events)


def test_child_listed_parents_not(bv, monkeypatch, tmp_path):
    """short lists that name the child's map byte and not its parents': an unlisted byte is four times ref"""
    use_path(monkeypatch, "streaming")
    vcf, trios = md.child_listed_parents_not_vcf()
    want = check(bv, vcf, ped(vcf, trios), tmp_path)
    forms = ctx_check(bv, vcf, want)
    assert all(forms[:8]) and not any(forms[8:])
    assert want["events"][0].tolist() == [0, 0, md.HET, md.REF, md.REF]


# ---- pedigree shapes

def test_child_precedes_its_parents(bv, bvcf_path, tmp_path):
    vcf, trios = md.pedigree_vcf(70, 23, 80, 9820, flip=0.08, miss=0.05, child_first=True)
    assert all(c < f and c < m for c, f, m in trios)
    want = check(bv, vcf, ped(vcf, trios), tmp_path)
    assert len(want["events"]) > 0


def test_child_and_parent_siblings_three_generations(bv, bvcf_path, tmp_path):
    """a random pedigree: samples that are a child in one trio and a parent in others, children that share parents"""
    vcf = pt.rare_vcf(129)
    trios = md.random_trios(129, 60, 9830)
    children, parents = {t[0] for t in trios}, [p for t in trios for p in t[1:]]
    assert children & set(parents) and len(set(parents)) < len(parents)
    want = check(bv, vcf, ped(vcf, trios), tmp_path)
    ctx_check(bv, vcf, want)


def test_zero_trios_and_no_sample_columns(bv, bvcf_path, tmp_path):
    vcf = pt.rare_vcf(65)
    names = pt.sample_names(vcf)
    for tag, fam in (("founders", md.fam_of([], names)), ("strangers", b"F a b c\nF d e f\n"), ("empty", b""),
                     ("duo", ("F %s %s 0\n" % (names[2], names[1])).encode())):
        rc, out, log, mendel, errors = run_with_mendel(bv, vcf, fam, tmp_path, tag=tag)
        assert rc == 0, log
        assert mendel == md.MENDEL_HEADER and errors == md.ERRORS_HEADER, tag
        assert out == orc.run(vcf)[1]
    sites = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    rc, out, log, mendel, errors = run_with_mendel(bv, sites, b"F a b c\n", tmp_path, tag="sites")
    assert rc == 0 and mendel == md.MENDEL_HEADER and errors == md.ERRORS_HEADER
    assert (out, log) == orc.run(sites)[1:3]
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, trios=[])  # no trios: nothing allocated or launched, and no counts
    ctx.process(data)
    info = ctx.trio_info()
    assert (info.n_trios, info.n_events, info.need_events) == (0, 0, 0) and not info.counts and not info.events
    ctx.reserve_trio_events(1 << 20)
    ctx.close()


def test_three_samples(bv, bvcf_path, tmp_path):
    """S = 3: one trio, one map byte"""
    vcf = pt.tiny_vcf(3, n_lines=60)
    want = check(bv, vcf, ped(vcf, [(1, 2, 0)]), tmp_path)
    ctx_check(bv, vcf, want)
    assert want["counts"].shape == (1, 3) and 0 < want["counts"][0, 2] < want["counts"][0, 1] < want["counts"][0, 0] < 60


def test_enable_trios_refuses_bad_indices(bv):
    for bad in ([(0, 1, 4)], [(0, 1, 2), (3, 3, 1)], [(2, 0, 2)]):
        with pytest.raises(bv.BvcfError) as ei:
            bv.Ctx(9 + 4, trios=bad)
        assert ei.value.rc == bv.E_ARG
    with pytest.raises(bv.BvcfError) as ei:
        bv.Ctx(9, trios=[(0, 1, 2)])  # no sample columns
    assert ei.value.rc == bv.E_ARG
    ctx = bv.Ctx(9 + 4)
    with pytest.raises(bv.BvcfError) as ei:
        ctx.trio_info()
    assert ei.value.rc == bv.E_ARG
    ctx.close()


# ---- composition: the reference is the oracle on the masked and cut text, minus the rows the gate takes out

def test_keep_samples_removes_a_parent(bv, bvcf_path, tmp_path):
    vcf, trios = md.pedigree_vcf(70, 23, 80, 9840, flip=0.08, miss=0.05)
    fam = ped(vcf, trios)
    gone = [trios[0][1], trios[5][2], trios[9][0]]  # a father, a mother, a child
    idx = [s for s in range(70) if s not in gone]
    cut = samplecut.cut_vcf(vcf, idx)
    want, body, log_o = oracle_side(cut, fam)
    assert len(want["trios"]) == 20
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx)
    for tag, cfg in (("keep", {"keepSamples": lst}),):
        rc, out, log, mendel, errors = run_with_mendel(bv, vcf, fam, tmp_path, cfg, tag=tag)
        assert rc == 0, log
        assert out == body and log == log_o
        assert mendel == want["mendel"] and errors == want["errors"], first_diff(errors, want["errors"])


def test_keep_samples_min_gq_and_gate(bv, bvcf_path, tmp_path):
    vcf = gtmask.seeded(pb.MASKED)
    ns = len(pt.sample_names(vcf))
    idx = sorted(random.Random(9300).sample(range(ns), 41))
    criteria = {"minMac": 2, "maxMissing": 0.2}
    st = {}
    cut = samplecut.cut_vcf(gtmask.mask_vcf(vcf, 20, 0, st), idx)
    assert st["masked"] > 100
    names = md.normalized(pt.sample_names(vcf))
    fam = md.fam_of(md.random_trios(ns, 40, 9850), names)
    rc_o, body, log_o, _ = orc.run(cut)
    assert rc_o == 0
    mask, counts, _ = sg.gate(body, len(idx), criteria)
    assert 0 < counts[1] < counts[0]
    kept = sg.kept_body(body, mask)
    want = md.expected_from_body(kept, pt.sample_names(cut), fam)
    assert 2 <= len(want["trios"]) < 40 and len(want["events"]) > 0
    assert (want["verdicts"] == md.UNINFORMATIVE).any()  # (masked calls are missing)
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx, eol=b"\r\n")
    cfg = dict(criteria, keepSamples=lst, minGQ=20)
    rc, out, log, mendel, errors = run_with_mendel(bv, vcf, fam, tmp_path, cfg)
    assert rc == 0, log
    assert out == kept and log == log_o
    assert mendel == want["mendel"], first_diff(mendel, want["mendel"])
    assert errors == want["errors"], first_diff(errors, want["errors"])


def test_with_and_without_plink_output(bv, bvcf_path, tmp_path):
    """the row index is shared: the .bed is what it is without the flags, the two files what they are without --plinkOutput"""
    vcf, trios = md.pedigree_vcf(129, 40, 100, 9860)
    fam = ped(vcf, trios)
    want = check(bv, vcf, fam, tmp_path)
    want_p = pb.expected(orc.run, vcf)[0]
    rc, out, log, _ = bv.run_buffer(vcf, {"plinkOutput": str(tmp_path / "alone")})
    assert rc == 0 and not pb.diff(pb.read_files(tmp_path / "alone"), want_p)
    rc, out, log, mendel, errors = run_with_mendel(bv, vcf, fam, tmp_path, {"plinkOutput": str(tmp_path / "set")}, tag="both")
    assert rc == 0, log
    assert not pb.diff(pb.read_files(tmp_path / "set"), want_p)
    assert mendel == want["mendel"] and errors == want["errors"]
    # and through a ctx with both enabled
    forms = ctx_check(bv, vcf, want, bed_rows=True)
    assert len(forms) * pb.row_bytes(129) == len(want_p["bed"]) - 3


def test_one_output_at_a_time(bv, monkeypatch, tmp_path):
    use_path(monkeypatch, "streaming")
    vcf, trios = md.pedigree_vcf(70, 23, 80, 9870, flip=0.08, miss=0.05)
    fam = tmp_path / "p.fam"
    fam.write_bytes(ped(vcf, trios))
    want, body, _ = oracle_side(vcf, ped(vcf, trios))
    for key in ("mendel", "mendelErrors"):
        path = tmp_path / key
        rc, out, log, _ = bv.run_buffer(vcf, {"fam": str(fam), key: str(path)})
        assert rc == 0 and out == body
        assert path.read_bytes() == want["mendel" if key == "mendel" else "errors"]
    assert sorted(os.listdir(tmp_path)) == ["mendel", "mendelErrors", "p.fam"]


# ---- arena growth: every row an error for every trio

def test_arena_growth_run_buffer(bv, bvcf_path, tmp_path):
    """30 000 events from 0.2 MB of text: they outrun the arena's max_batch_bytes / 64 and process_block grows it"""
    vcf, trios = md.all_errors_vcf(100, 300)
    want = check(bv, vcf, ped(vcf, trios), tmp_path, max_batch_bytes=1 << 20)
    assert len(want["events"]) == 30000 > (1 << 20) // 64


def test_arena_growth_ctx(bv):
    """the same through a ctx: BVCF_E_CAPACITY with the need reported, bvcf_reserve_trio_events, the batch again"""
    vcf, trios = md.all_errors_vcf(100, 300)
    want = oracle_side(vcf, ped(vcf, trios))[0]
    nh, eol, data = split_file(vcf)
    ctx = bv.Ctx(nh, max_batch_bytes=1 << 20, trios=want["trios"])
    with pytest.raises(bv.BvcfError) as ei:
        ctx.process(data)
    assert ei.value.rc == bv.E_CAPACITY
    info = ctx.trio_info()
    assert info.need_events == 30000 and info.n_events == 0 and not info.events and not info.counts
    ctx.reserve_trio_events(info.need_events)
    ctx.process(data)
    counts, events = ctx.trio_stats()
    ctx.close()
    assert np.array_equal(events, want["events"]) and np.array_equal(counts.astype(np.uint64), want["counts"])


def cli(args, stdin_bytes=None, timeout=300):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout)


def test_arena_growth_cli(bv, tmp_path):
    vcf, trios = md.all_errors_vcf(100, 1800)  # 1.1 MB: two batches under --batchMB 1
    assert len(vcf) > (1 << 20)
    fam = ped(vcf, trios)
    want, out_o, _ = oracle_side(vcf, fam)
    src, f = tmp_path / "e.vcf", tmp_path / "e.fam"
    src.write_bytes(vcf)
    f.write_bytes(fam)
    for tag, extra in (("one", []), ("two", ["--devices", "0,0"])):
        m, e = tmp_path / (tag + ".mendel"), tmp_path / (tag + ".errors")
        p = cli(["--in", str(src), "--batchMB", "1", "--fam", str(f), "--mendel", str(m), "--mendelErrors", str(e)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        assert m.read_bytes() == want["mendel"] and e.read_bytes() == want["errors"], tag


# ---- the Ctx

@pytest.mark.parametrize("path", ["1", "2"])
def test_ctx_many_batches(bv, monkeypatch, path):
    """more batches than slots, two in flight: trio_stats() is the batch collected last; the batches' tables add up to the
    file's and their events, rows renumbered, are the file's"""
    monkeypatch.setenv("BVCF_PATH", path)
    vcf, trios = md.pedigree_vcf(299, 90, 600, 9880)
    want = oracle_side(vcf, ped(vcf, trios))[0]
    nh, eol, data = split_file(vcf)
    lines = data.split(b"\n")[:-1]
    blocks = [b"".join(x + b"\n" for x in lines[i:i + 45]) for i in range(0, len(lines), 45)]
    assert len(blocks) > 6
    ctx = bv.Ctx(nh, n_slots=2, trios=want["trios"], want_class_maps=False)
    total = np.zeros((90, 3), dtype=np.uint64)
    events, row0 = [], 0

    def take():
        nonlocal total, row0
        b = ctx.collect()
        assert len(b.cmap) == 0  # (the maps stay on the device)
        counts, ev = ctx.trio_stats()
        total += counts
        ev = ev.copy()
        ev[:, 0] += row0
        events.append(ev)
        row0 += len(row_forms(bv, b))

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
    assert np.array_equal(total, want["counts"])
    assert np.array_equal(np.concatenate(events), want["events"])


# ---- the CLI (each run under its own time limit)

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("mendel")
    vcf = vcfgen.gen_vcf(41, 3000, 401, weird=0.02) + vcfgen.gen_vcf(42, 1500, 401, weird=0.02).split(b"\n", 3)[3]
    names = md.normalized(pt.sample_names(vcf))
    fam = md.fam_of(md.random_trios(401, 130, 9890), names, sep=" ", eol="\r\n")
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz", "fam": d / "c.fam"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    paths["fam"].write_bytes(fam)
    want, out_o, _ = md.expected(orc.run, vcf, fam)
    return vcf, paths, d, out_o, want, fam


def mendel_args(d, tag, fam):
    return ["--fam", str(fam), "--mendel", str(d / (tag + ".mendel")), "--mendelErrors", str(d / (tag + ".errors"))]


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d, out_o, want, _ = cohort
    assert len(want["trios"]) > 100 and len(want["events"]) > 1000
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("devices00", ["--in", str(paths["text"]), "--devices", "0,0"], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-devices00", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", "0,0"], None)]
    for tag, args, stdin in runs:
        p = cli(args + mendel_args(d, tag, paths["fam"]), stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        assert p.stdout.split(b"\n", 1)[1] == out_o, tag
        assert (d / (tag + ".mendel")).read_bytes() == want["mendel"], tag
        assert (d / (tag + ".errors")).read_bytes() == want["errors"], tag


def test_cli_no_out_qc_pass(bv, cohort):
    vcf, paths, d, out_o, want, _ = cohort
    for tag, src, keys in (("noout-text", "text", ("mendel", "errors")), ("noout-bgzf", "bgzf", ("mendel",)), ("noout-e", "text", ("errors",))):
        args = ["--in", str(paths[src]), "--noOut", "--fam", str(paths["fam"])]
        for k in keys:
            args += ["--mendel" if k == "mendel" else "--mendelErrors", str(d / ("%s.%s" % (tag, k)))]
        p = cli(args)
        assert p.returncode == 0, p.stderr[-400:]
        assert p.stdout == b""
        for k in keys:
            assert (d / ("%s.%s" % (tag, k))).read_bytes() == want[k], (tag, k)


def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d, out_o, want, fam = cohort
    outs = {}
    for tag, extra in (("plain", []), ("fam-only", ["--fam", str(d / "no_such_file.fam")]), ("mendel", mendel_args(d, "o", paths["fam"]))):
        f = {k: d / ("%s.%s" % (tag, k)) for k in ("tsv.gz", "arrow", "samples", "stats", "pairs", "report")}
        prefix = d / ("%s.plink" % tag)
        p = cli(["--in", str(paths["bgzf"]), "--out", str(f["tsv.gz"]), "--compressOutput", "bgzf", "--dosageOutput", str(f["arrow"]),
                 "--sample", str(f["samples"]), "--sampleStats", str(f["stats"]), "--relatedness", str(f["pairs"]),
                 "--minMac", "3", "--siteFilterReport", str(f["report"]), "--plinkOutput", str(prefix)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        outs[tag] = tuple(hashlib.sha256(x.read_bytes()).hexdigest() for x in f.values()) + \
            tuple(hashlib.sha256(x).hexdigest() for x in pb.read_files(prefix).values()) + (p.stderr,)
    assert outs["plain"] == outs["fam-only"] == outs["mendel"]  # (--fam alone: accepted, ignored, not even opened)
    # (with the gate: the rows counted are the rows of that TSV)
    mask, _, _ = sg.gate(out_o, 401, {"minMac": 3})
    gated = md.expected_from_body(sg.kept_body(out_o, mask), pt.sample_names(vcf), fam)
    assert (d / "o.mendel").read_bytes() == gated["mendel"] and (d / "o.errors").read_bytes() == gated["errors"]


def test_cli_pedigree_errors(bv, tmp_path):
    vcf = pt.rare_vcf(63)
    names = pt.sample_names(vcf)
    two = vcfgen.header(3, names=["A", "B", "B"]).encode() + pt.snp_line(100, ["0|1", "0|0", "1|1"]).encode()
    cases = [("short", vcf, "F %s %s %s\nF x\n" % tuple(names[:3]), [b"line 2"]),
             ("dup", vcf, "F %s %s %s\nF %s 0 0\nG %s 0 0\n" % (names[0], names[1], names[2], names[5], names[0]), [names[0].encode(), b"line 3"]),
             ("same", vcf, "F %s %s %s\n" % (names[4], names[7], names[7]), [names[4].encode()]),
             ("ambiguous", two, "F A B 0\n", [b'"A"'])]
    for tag, text, fam, must in cases:
        f, m, e = tmp_path / (tag + ".fam"), tmp_path / (tag + ".mendel"), tmp_path / (tag + ".errors")
        f.write_text(fam)
        p = cli(["--fam", str(f), "--mendel", str(m), "--mendelErrors", str(e)], text)
        assert p.returncode == 1 and p.stderr.count(b"\n") == 1, (tag, p.stderr)
        assert all(x in p.stderr for x in must), (tag, p.stderr)
        assert m.read_bytes() == b"" and e.read_bytes() == b""  # (opened first, written only after a successful run)
    p = cli(["--fam", str(tmp_path / "missing.fam"), "--mendel", str(tmp_path / "x.mendel")], vcf)
    assert p.returncode == 1 and p.stderr.count(b"\n") == 1 and b"missing.fam" in p.stderr


# ---- the golden 1KG slice, a pedigree made up over its 2 504 names

def test_golden_1kg(bv, golden_1kg, monkeypatch, tmp_path):
    """800 trios over 2 504 unrelated samples: nearly every carrier row contradicts somebody.  The table byte for byte and the
    number of events (the list runs to hundreds of thousands of lines: its text is compared on the smaller inputs)"""
    vcf = golden_1kg[0]
    names = md.normalized(pt.sample_names(vcf))
    assert len(names) == 2504
    fam = md.fam_of(md.random_trios(2504, 800, 9900), names)
    want, out_o, log_o = md.expected(orc.run, vcf, fam, with_errors_text=False)
    assert len(want["trios"]) == 800 and len(want["events"]) > 100000
    head = md.errors_text(want["events"][:2000], out_o, want["trios"], want["names"])
    for path in ("streaming", "census"):
        use_path(monkeypatch, path)
        rc, out, log, mendel, errors = run_with_mendel(bv, vcf, fam, tmp_path, tag=path)
        assert rc == 0, log
        assert out == out_o and log == log_o
        assert mendel == want["mendel"], first_diff(mendel, want["mendel"])
        assert errors.count(b"\n") == 1 + len(want["events"])
        assert errors[:len(head)] == head
