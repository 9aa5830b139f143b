"""--mendel / --mendelErrors without a device: the exported verdict (bvcf_trio_verdict, the function the trio kernels
run) and .fam parser (bvcf_parse_fam), the layout and the markers of the config, the CLI's argument checks, and -- with
the oracle alone -- that the inputs of tests/test_gpu_mendel.py hold what the cases are about.  The reference verdict and
parser are mendel.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mendel as md
import oracle_lib as orc
import pairtable as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


# ---- the verdict

def test_verdict_of_all_64_class_triples(bv):
    kinds = {}
    for c in range(4):
        for f in range(4):
            for m in range(4):
                got = bv.trio_verdict(c, f, m)
                assert got == md.verdict(c, f, m), (c, f, m)
                kinds[got] = kinds.get(got, 0) + 1
    # 27 informative triples: 15 consistent, 2 de novo, 10 other errors
    assert kinds == {bv.TRIO_UNINFORMATIVE: 37, bv.TRIO_CONSISTENT: 15, bv.TRIO_DENOVO: 2, bv.TRIO_ERROR: 10}
    assert (bv.TRIO_UNINFORMATIVE, bv.TRIO_CONSISTENT, bv.TRIO_DENOVO, bv.TRIO_ERROR) == (md.UNINFORMATIVE, md.CONSISTENT, md.DENOVO, md.ERROR)
    assert bv.trio_verdict(4, 0, 0) == -1 and bv.trio_verdict(0, 0, 9) == -1


def test_reference_verdict_by_hand():
    R, H, O, M = md.REF, md.HET, md.HOM, md.MISSING
    assert md.verdict(H, R, R) == md.DENOVO and md.verdict(O, R, R) == md.DENOVO
    assert md.verdict(R, R, R) == md.CONSISTENT and md.verdict(H, H, R) == md.CONSISTENT and md.verdict(O, H, H) == md.CONSISTENT
    assert md.verdict(R, O, R) == md.ERROR and md.verdict(O, H, R) == md.ERROR and md.verdict(H, O, O) == md.ERROR
    assert md.verdict(R, O, H) == md.ERROR and md.verdict(H, O, H) == md.CONSISTENT
    assert md.verdict(M, R, R) == md.UNINFORMATIVE and md.verdict(H, R, M) == md.UNINFORMATIVE


def test_multiallelic_collapse_keeps_consistent_trios_consistent():
    """a trio that is consistent on a line with three alleles is consistent in every "this ALT against the rest" row"""
    alleles = range(3)
    for f in [(a, b) for a in alleles for b in alleles]:
        for m in [(a, b) for a in alleles for b in alleles]:
            for c in [(a, b) for a in f for b in m]:  # every child the parents can have
                for alt in (1, 2):
                    cls = [sum(x == alt for x in g) for g in (c, f, m)]
                    assert md.verdict(*cls) == md.CONSISTENT, (c, f, m, alt)


# ---- the .fam parser

NAMES = [b"kid", b"dad", b"mum", b"sis", b"gran", b"gramps", b"twin", b"twin", b"0"]


def both(bv, text, names=NAMES):
    """(the library's result, the reference's) in one form: ("ok", trios) or ("bad", why, line, iid)"""
    got = bv.parse_fam(text, names)
    got = ("ok", got[1]) if got[0] == bv.FAM_OK else ("bad",) + tuple(got)
    try:
        want = ("ok", md.parse_fam(text, names))
    except md.FamError as e:
        want = ("bad", e.why, e.line, e.iid)
    return got, want


GOOD = {
    "plain": b"F kid dad mum 1 -9\nF dad gramps gran 1 -9\nF mum 0 0 2 -9\nF sis dad mum\n",
    "four fields, CRLF, blanks and TAB runs, empty lines": b"F  kid \t dad\tmum\r\n\r\n\nF\t\tsis dad  mum  \r\n   \n",
    "no trailing newline": b"F sis dad mum 2 -9",
    "child before its parents in the file and the header": b"F sis dad mum\nF kid dad mum\n",
    "a larger cohort: unknown individuals and unknown parents": b"F other a b\nF kid dad stranger\nF sis stranger mum\nF mum dad gran\n",
    "a parent that is none": b"F kid 0 mum\nF sis dad 0\nF dad 0 0\n",
    "the name 0 as a parent is none, as an individual a sample": b"F 0 dad mum\nF kid 0 mum\n",
    "three generations, a child that is a parent": b"F dad gramps gran\nF kid dad mum\n",
    "an ambiguous name on an ignored line": b"F nobody twin dad\n",
    "the same sample twice without a trio": b"F kid kid 0\nF sis sis stranger\n",
    "empty": b"",
    "a duplicate of somebody who is no sample": b"F x a b\nF x a b\n",
}
BAD = {
    "one field": (b"F kid dad mum\nkid\n", md.FAM_SHORT_LINE, 2),
    "three fields": (b"\nF kid dad\n", md.FAM_SHORT_LINE, 2),
    "three fields of somebody unknown": (b"F x y\n", md.FAM_SHORT_LINE, 1),
    "an individual on two lines": (b"F kid dad mum\nF sis dad mum\nG kid 0 0\n", md.FAM_DUP_IID, 3),
    "an individual matching two columns": (b"F twin dad mum\n", md.FAM_AMBIGUOUS, 1),
    "a parent matching two columns": (b"F kid dad mum\nF sis twin mum\n", md.FAM_AMBIGUOUS, 2),
    "a parent matching two columns, the other none": (b"F sis 0 twin\n", md.FAM_AMBIGUOUS, 1),
    "child is its father": (b"F kid kid mum\n", md.FAM_SAME_SAMPLE, 1),
    "child is its mother": (b"F kid dad kid\n", md.FAM_SAME_SAMPLE, 1),
    "father is mother": (b"F sis dad dad\r\n", md.FAM_SAME_SAMPLE, 1),
}


@pytest.mark.parametrize("name", list(GOOD))
def test_parse_fam_good_files(bv, name):
    got, want = both(bv, GOOD[name])
    assert got == want and got[0] == "ok", (got, want)


def test_parse_fam_good_files_by_hand(bv):
    assert bv.parse_fam(GOOD["plain"], NAMES) == (0, [(0, 1, 2), (1, 5, 4), (3, 1, 2)])
    assert bv.parse_fam(GOOD["a larger cohort: unknown individuals and unknown parents"], NAMES) == (0, [(2, 1, 4)])
    assert bv.parse_fam(GOOD["the name 0 as a parent is none, as an individual a sample"], NAMES) == (0, [(8, 1, 2)])
    assert bv.parse_fam(GOOD["plain"], []) == (0, []) and bv.parse_fam(b"", NAMES) == (0, [])


@pytest.mark.parametrize("name", list(BAD))
def test_parse_fam_error_rules(bv, name):
    text, why, line = BAD[name]
    got, want = both(bv, text)
    assert got == want, (got, want)
    assert got[:3] == ("bad", why, line), got
    assert (got[3] is None) == (why == md.FAM_SHORT_LINE)


def test_parse_fam_pedigrees_of_the_gpu_cases(bv):
    for name, (vcf, fam) in md.fuzz_inputs().items():
        names = [n.encode() for n in md.normalized(pt.sample_names(vcf))]
        got, want = both(bv, fam, names)
        assert got == want and got[0] == "ok" and len(got[1]) >= 2, name
    trios = md.random_trios(300, 100, 5)
    names = ["N%d" % i for i in range(300)]
    for sep, eol in (("\t", "\n"), (" ", "\r\n"), (" \t ", "\n")):
        fam = md.fam_of(trios, names, extra_lines=["F9 ghost N1 N2 0 -9"], sep=sep, eol=eol)
        assert bv.parse_fam(fam, [n.encode() for n in names]) == (0, trios)
    # a sample that is a child and a parent, and siblings, are in there
    children, parents = {t[0] for t in trios}, {p for t in trios for p in t[1:]}
    assert children & parents and len(parents) < 2 * len(trios)


# ---- the config

def test_header_binding_and_library_agree(bv):
    with open(os.path.join(ROOT, "include", "bvcf.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "bvcf_plan.h")) as f:
        plan = f.read()
    with open(os.path.join(ROOT, "include", "bvcf_bench.h")) as f:
        bench = f.read()
    assert re.search(r"int bvcf_enable_trios\(bvcf_ctx \*ctx, const uint32_t \*trios .*, uint32_t n\);", h)
    assert re.search(r"int bvcf_reserve_trio_events\(bvcf_ctx \*ctx, uint64_t n\);", h)
    assert re.search(r"int bvcf_trio_stats\(const bvcf_ctx \*ctx, bvcf_trio_info \*out\);", h)
    assert "#define BVCF_CONFIG_MORE_TRIOS 3\n" in h and bv.CONFIG_MORE_TRIOS == 3 > bv.CONFIG_MORE_PLINK
    assert re.search(r"int bvcf_trio_verdict\(uint32_t child, uint32_t father, uint32_t mother\);", plan)
    assert "int bvcf_parse_fam(" in plan and "bvcf_bench_trio_kernels" in bench
    for name in ("bvcf_enable_trios", "bvcf_reserve_trio_events", "bvcf_trio_stats", "bvcf_config_trios_defaults"):
        assert name in bv.EXPORTS and hasattr(bv.lib, name)
    for name in ("bvcf_trio_verdict", "bvcf_parse_fam"):
        assert name in bv.PLAN_EXPORTS and hasattr(bv.lib, name)
    assert "bvcf_bench_trio_kernels" in bv.BENCH_EXPORTS and hasattr(bv.lib, "bvcf_bench_trio_kernels")
    assert "\t".join(bv.MENDEL_COLUMNS).encode() + b"\n" == md.MENDEL_HEADER
    assert "\t".join(bv.MENDEL_ERRORS_COLUMNS).encode() + b"\n" == md.ERRORS_HEADER
    assert bv.ABI_VERSION == 9 and bv.ABI_VERSION_SUBSET == 10  # no ABI version change


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    paths = ["more", "fam_path", "mendel_path", "mendel_errors_path"]
    info = ["counts", "events", "n_events", "need_events", "n_trios", "reserved"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\nint main(){'
                   'printf("%zu %zu %zu %zu", sizeof(bvcf_config_more), offsetof(bvcf_config_more, plink_prefix),'
                   "sizeof(bvcf_config_trios), sizeof(bvcf_trio_info));"
                   + "".join('printf(" %%zu", offsetof(bvcf_config_trios, %s));' % f for f in paths)
                   + "".join('printf(" %%zu", offsetof(bvcf_trio_info, %s));' % f for f in info)
                   + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M, T, I = bv.ConfigMore, bv.ConfigTrios, bv.TrioInfo
    assert out == [C.sizeof(M), M.plink_prefix.offset, C.sizeof(T), C.sizeof(I)] + [getattr(T, f).offset for f in paths] + \
        [getattr(I, f).offset for f in info]
    # bvcf_config_more keeps its size, plink_prefix is still its last field, and the new struct begins with one
    assert C.sizeof(M) == M.plink_prefix.offset + 8 == 184 and T.more.offset == 0 and T.fam_path.offset == C.sizeof(M)
    assert C.sizeof(T) == C.sizeof(M) + 24


def test_older_defaults_write_nothing_new(bv):
    """the three older *_defaults, called on the head of the larger struct, leave what is behind bvcf_config_more alone --
    and each still stops where it stopped"""
    M = bv.ConfigMore
    for fn, first_untouched in ((bv.lib.bvcf_config_more_defaults, M.site_gate.offset),
                                (bv.lib.bvcf_config_gate_defaults, M.plink_prefix.offset),
                                (bv.lib.bvcf_config_plink_defaults, C.sizeof(M))):
        t = bv.ConfigTrios()
        C.memset(C.byref(t), 0xFF, C.sizeof(t))
        fn(C.byref(t))
        assert bytes(t)[first_untouched:] == b"\xff" * (C.sizeof(t) - first_untouched), fn
    t = bv.ConfigTrios()
    C.memset(C.byref(t), 0xFF, C.sizeof(t))
    bv.lib.bvcf_config_plink_defaults(C.byref(t))
    assert t.more.base.reserved[1] == bv.CONFIG_MORE_PLINK
    bv.lib.bvcf_config_trios_defaults(C.byref(t))
    assert (t.more.base.reserved[0], t.more.base.reserved[1]) == (bv.CONFIG_MORE, bv.CONFIG_MORE_TRIOS)
    assert t.fam_path is None and t.mendel_path is None and t.mendel_errors_path is None and t.more.plink_prefix is None
    g = t.more.site_gate
    assert (g.size, g.min_mac, g.min_maf, g.max_maf, g.max_missing, g.hwe_p) == (40, 0, 0.0, 1.0, 1.0, 0.0)


def test_make_config_markers(bv):
    """the larger struct and marker 3 only with --mendel / --mendelErrors; every other config comes out as before"""
    assert list(bv.make_config({}).reserved) == [0, 0]
    assert list(bv.make_config({"fam": "/x/f"}).reserved) == [0, 0]
    assert list(bv.make_config({"fam": "/x/f", "relatedness": "/x"}).reserved) == [bv.CONFIG_MORE, 0]
    assert list(bv.make_config({"fam": "/x/f", "minMac": 2}).reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_GATE]
    assert list(bv.make_config({"fam": "/x/f", "plinkOutput": "/x/p"}).reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_PLINK]
    for cfg in ({"fam": "/x/f", "mendel": "/x/m"}, {"fam": "/x/f", "mendelErrors": "/x/e", "minMaf": 0.05, "plinkOutput": "/x/p"}):
        c = bv.make_config(cfg)
        assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_TRIOS]
        t = C.cast(C.byref(c), C.POINTER(bv.ConfigTrios)).contents
        assert t.fam_path == b"/x/f"
        assert t.mendel_path == (cfg["mendel"].encode() if "mendel" in cfg else None)
        assert t.mendel_errors_path == (cfg["mendelErrors"].encode() if "mendelErrors" in cfg else None)
        assert t.more.plink_prefix == (cfg["plinkOutput"].encode() if "plinkOutput" in cfg else None)
        assert t.more.site_gate.size == 40 and t.more.site_gate.min_maf == cfg.get("minMaf", 0.0) and t.more.site_gate.max_maf == 1.0


SITES = (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
         b"chr1\t100\t.\tA\tC\t50\tPASS\t.\n")


def run_marked(bv, cfg, marker):
    """bvcf_run_buffer over a ConfigTrios with base.reserved[1] = marker -> the log.  The two files are opened before any
    device work, so this says which marker reads the fields with or without a device"""
    c = bv.make_config(cfg)
    c.reserved[1] = marker
    return bv.run_buffer(SITES, c)[2]


def test_marker_levels_are_read_as_specified(bv, tmp_path):
    fam = tmp_path / "p.fam"
    fam.write_bytes(b"F a b c\n")
    bad = tmp_path / "no_such_dir" / "m.tsv"
    for key in ("mendel", "mendelErrors"):
        cfg = {"fam": str(fam), key: str(bad)}
        # marker 3: the path is read, and an unwritable one is one message
        log = run_marked(bv, cfg, bv.CONFIG_MORE_TRIOS)
        assert ("open %s: " % bad) in log and log.count("\n") == 1, log
        # marker 2 and below: nothing behind plink_prefix is read
        for marker in (bv.CONFIG_MORE_PLINK, bv.CONFIG_MORE_GATE, 0):
            assert str(bad) not in run_marked(bv, cfg, marker)
        good = tmp_path / ("good_" + key)
        for marker in (bv.CONFIG_MORE_PLINK, bv.CONFIG_MORE_GATE, 0):
            run_marked(bv, {"fam": str(fam), key: str(good)}, marker)
            assert not os.path.exists(good)
        run_marked(bv, {"fam": str(fam), key: str(good)}, bv.CONFIG_MORE_TRIOS)
        assert os.path.exists(good)
    # marker 3 still reaches the older fields ("at least"): the prefix is read
    log = run_marked(bv, {"fam": str(fam), "mendel": str(tmp_path / "m"), "plinkOutput": str(tmp_path / "no_such_dir" / "p")},
                     bv.CONFIG_MORE_TRIOS)
    assert "no_such_dir/p.bed" in log and log.count("\n") == 1, log
    # a run that asks for a table without a pedigree is refused before any device work
    c = bv.make_config({"mendel": str(tmp_path / "m2")})
    rc, _, log, _ = bv.run_buffer(SITES, c)
    assert rc != 0 and "fam" in log and log.count("\n") == 1


# ---- the CLI's argument checks (no device is reached)

def cli(args, stdin_bytes=b""):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=60)


def test_cli_flags_without_a_value_or_a_pedigree(tmp_path):
    for flag in ("mendel", "mendelErrors"):
        p = cli(["--" + flag])
        assert p.returncode == 2 and ("flag needs an argument: -%s" % flag).encode() in p.stderr and p.stderr.count(b"\n") == 1
        assert p.stdout == b""
        p = cli(["--%s=" % flag, "--fam", "x.fam"])
        assert p.returncode == 2 and p.stderr.count(b"\n") == 1 and p.stdout == b""
        p = cli(["--" + flag, str(tmp_path / "out.tsv")])
        assert p.returncode == 2 and b"-fam" in p.stderr and p.stderr.count(b"\n") == 1 and p.stdout == b""
        assert not os.path.exists(tmp_path / "out.tsv")
    p = cli(["--noOut", "--fam", "x.fam"])  # --fam alone is still no output
    assert p.returncode == 1 and b"When specifying --noOut" in p.stderr


def test_cli_unwritable_paths(tmp_path):
    fam = tmp_path / "p.fam"
    fam.write_bytes(b"F a b c\n")
    bad = tmp_path / "no_such_dir" / "m.tsv"
    for flag in ("mendel", "mendelErrors"):
        p = cli(["--fam", str(fam), "--" + flag, str(bad)], SITES)
        assert p.returncode == 1 and p.stderr.count(b"\n") == 1 and str(bad).encode() in p.stderr and p.stdout == b""


# ---- the inputs of tests/test_gpu_mendel.py, with the oracle alone

@pytest.fixture(scope="module")
def covered():
    out = {}
    for name, (vcf, fam) in md.gpu_inputs().items():
        rc, body, _, _ = orc.run(vcf)
        assert rc == 0
        names = md.normalized(pt.sample_names(vcf))
        trios = md.parse_fam(fam, [n.encode() for n in names])
        cls = md.classes_of(*pt.matrices(body, names))
        v, cfm = md.verdicts(cls, trios)
        out[name] = (md.coverage(v, cfm), cls, trios, v)
    return out


def test_every_seeded_gpu_input_shows_all_four_verdicts(covered):
    """every seeded input of the GPU cases: a de novo call, another error, an uninformative and a consistent verdict.  (The
    crafted files say what they hold where they are made: all_errors_vcf is errors only, by design.)"""
    assert len(covered) >= 10
    for name, ((kinds, _), cls, trios, v) in covered.items():
        assert kinds == {md.UNINFORMATIVE, md.CONSISTENT, md.DENOVO, md.ERROR}, (name, kinds)
        assert len(trios) >= 2


def test_gpu_inputs_together_cover_all_27_informative_triples(covered):
    seen = set()
    for (_, triples), _, _, _ in covered.values():
        seen |= triples
    assert seen == set(md.INFORMATIVE_TRIPLES) and len(seen) == 27
    # the crafted file alone shows every triple to every trio
    (_, triples), _, trios, v = covered["triples"]
    assert triples == set(md.INFORMATIVE_TRIPLES) and len(trios) == 27


def test_pedigree_inputs_hold_short_list_and_dense_rows_with_events(covered):
    for name in ("ped300", "chunk130"):
        _, cls, trios, v = covered[name]
        carriers = ((cls == md.HET) | (cls == md.HOM) | (cls == md.MISSING)).sum(axis=1)
        has_event = (v >= md.DENOVO).any(axis=1)
        ns = cls.shape[1]
        assert (has_event & (carriers <= 15)).any() and (has_event & (8 * carriers >= ns)).any(), name


def test_all_errors_input_outruns_the_starting_arena():
    vcf, trios = md.all_errors_vcf(100, 300)
    # --batchMB 1: the arena starts at 2^20 / 64 = 16 384 events
    assert len(vcf) < (1 << 20) and 100 * 300 > (1 << 20) // 64
    rc, body, _, _ = orc.run(vcf)
    want = md.expected_from_body(body, pt.sample_names(vcf), md.fam_of(trios, pt.sample_names(vcf)))
    assert rc == 0 and len(want["events"]) == 30000 and (want["counts"] == [300, 300, 300]).all()  # (both parents ref: de novo)


def test_child_listed_parents_not_input():
    vcf, trios = md.child_listed_parents_not_vcf()
    rc, body, _, _ = orc.run(vcf)
    assert rc == 0
    want = md.expected_from_body(body, pt.sample_names(vcf), md.fam_of(trios, pt.sample_names(vcf)))
    ev = want["events"]
    assert want["trios"] == sorted(trios)
    # rows 0 and 1: child 8 het / hom, parents (map bytes 25 and 50) not listed -> de novo
    assert ev[0].tolist()[:2] == [0, 0] and ev[0].tolist()[2:] == [md.HET, md.REF, md.REF]
    assert ev[1].tolist()[2:] == [md.HOM, md.REF, md.REF]


def test_file_texts_by_hand():
    body = b"chr1\t5\tSNP\tA\tG\t1\tk\t0.5\t!\t0\t!\t0\t1\t4\t0.25\n"
    want = md.expected_from_body(body, ["k", "d", "m"], b"F k d m\n")
    assert want["mendel"] == md.MENDEL_HEADER + b"k\td\tm\t1\t1\t1\t1\n"
    assert want["errors"] == md.ERRORS_HEADER + b"chr1\t5\tA\tG\tk\td\tm\thet\tref\tref\tdenovo\n"
    none = md.expected_from_body(b"", ["k", "d", "m"], b"F k d m\n", {"emptyField": "NA"})
    assert none["mendel"] == md.MENDEL_HEADER + b"k\td\tm\t0\t0\t0\tNA\n" and none["errors"] == md.ERRORS_HEADER
    assert md.mendel_text(np.array([[3, 1, 0], [7, 0, 0]]), [(0, 1, 2), (2, 0, 1)], ["a", "b", "c"]) == \
        md.MENDEL_HEADER + b"a\tb\tc\t3\t1\t0\t0.333\nc\ta\tb\t7\t0\t0\t0\n"
