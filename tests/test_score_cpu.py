"""--score without a device: the weight grammar and its rounding, the limbs, the exact decimal text, the score file's rules
and the table's probe agree with the definition written in Python (score.py); the structs match the header; the CLI refuses
what it must; the GPU tests' inputs reach every case; and bvcf_score_q.h -- the arithmetic the kernels, the table builder and
the writer share -- runs clean in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as orc
import pairtable as pt
import score
import variantlist as vl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bystro-vcf_amd", "csrc")
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def both(bv, text):
    """(reference, library): ("ok", W) / ("bad",) / ("big",)"""
    out = []
    for fn in (score.weight, bv.score_weight):
        try:
            out.append(("ok", fn(text)))
        except ValueError:
            out.append(("bad",))
        except OverflowError:
            out.append(("big",))
    return tuple(out)


# ---- a weight

WORKED = [(b"0.0000000000005", 1), (b"-0.0000000000005", -1), (b"4.9999e-13", 0), (b"1e6", 10 ** 18), (b"-1E+6", -10 ** 18),
          (b"0", 0), (b"-0", 0), (b"+.5", 5 * 10 ** 11), (b"5.", 5 * 10 ** 12), (b"1.5e-12", 2), (b"2.5e-12", 3), (b"-2.5e-12", -3),
          (b"0.4999999999995", 5 * 10 ** 11), (b"0.49999999999949999", 499999999999), (b"1e-999", 0), (b"0e999", 0),
          (b"000000000000000000000000000000000000000000000000000000000001.5", 15 * 10 ** 11),
          (b"1000000.0000000000004999", 10 ** 18), (b"999999.9999999999995", 10 ** 18), (b"1e-12", 1), (b"12345678.9e-2", 123456789 * 10 ** 9)]
REFUSED_BIG = [b"1000000.000000000001", b"1000000.0000000000005", b"1e7", b"1e999", b"-1000001", b"9" * 64]
REFUSED_BAD = [b"", b".", b"+", b"-", b"e5", b"1e", b"1e+", b"1e1234", b" 1", b"1 ", b"nan", b"inf", b"-inf", b"0x10", b"1,5", b"1..5",
               b"1e5.0", b"--1", b"1_0", b"1" * 65, b"0." + b"0" * 63, b"\t1"]


def test_worked_cases_ties_and_bounds(bv):
    for text, w in WORKED:
        assert both(bv, text) == (("ok", w), ("ok", w)), text
    for text in REFUSED_BIG:
        assert both(bv, text) == (("big",), ("big",)), text
    for text in REFUSED_BAD:
        assert both(bv, text) == (("bad",), ("bad",)), text


def other_texts():
    """the texts of the --pheno value tests: the two parsers are one function with two range rules"""
    import test_assoc_cpu as other
    return [t for t, _ in other.WORKED] + other.REFUSED_BIG + other.REFUSED_BAD


def test_the_value_tests_texts_by_the_weight_rule(bv):
    """a text a hair above 10^6 is a weight -- the bound is on the rounded W -- though it is no phenotype value"""
    verdicts = {t: both(bv, t) for t in other_texts()}
    for t, (a, b) in verdicts.items():
        assert a == b, t
    assert verdicts[b"1000000.000000000000000001"][0] == ("ok", 10 ** 18) and verdicts[b"1000000.0000001"][0] == ("big",)
    assert verdicts[b"999999.9999995"][0] == ("ok", 9999999999995 * 10 ** 5) and verdicts[b"0.0000005"][0] == ("ok", 500000)


def seeded_texts(n, seed=1):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        if rng.random() < 0.3:  # any bytes of the grammar's alphabet
            out.append(bytes(rng.choice(b"0123456789.eE+-") for _ in range(rng.randint(1, 14))))
            continue
        ip = "".join(rng.choice("0123456789") for _ in range(rng.choice([0, 0, 1, 1, 2, 6, 7, 8, 19])))
        fp = "".join(rng.choice("0123456789") for _ in range(rng.choice([0, 1, 5, 11, 12, 13, 14, 20, 30])))
        if rng.random() < 0.2:  # a tie, or next to one
            fp = (fp[:12] + "0" * 12)[:12] + rng.choice(["5", "50", "49", "51", "4" + "9" * 10, "5" + "0" * 10 + "1"])
        ex = rng.choice(["", "", "e%d" % rng.randint(-25, 8), "E+%d" % rng.randint(0, 7), "e-%03d" % rng.randint(0, 30)])
        point = "." if fp else rng.choice(["", "."])
        out.append((rng.choice(["", "-", "+"]) + ip + point + fp + ex).encode())
    return out


def test_parser_against_fractions(bv):
    texts = seeded_texts(6000)
    verdicts = [both(bv, t) for t in texts]
    for t, (a, b) in zip(texts, verdicts):
        assert a == b, t
    kinds = [a[0] for a, _ in verdicts]
    assert kinds.count("ok") > 2000 and kinds.count("bad") > 500 and kinds.count("big") > 100
    assert sum(1 for a, _ in verdicts if a[0] == "ok" and a[1] < 0) > 500


def test_limbs_round_trip(bv):
    rng = random.Random(2)
    ws = [0, 1, -1, 127, -128, 128, -129, 10 ** 18, -10 ** 18, 10 ** 18 - 1]
    for n in range(1, 9):  # the largest and smallest W of n limbs, and the first past them
        top = sum(127 << (8 * a) for a in range(n))
        bot = -sum(128 << (8 * a) for a in range(n))
        ws += [w for w in (top, bot, top + 1, bot - 1) if abs(w) <= 10 ** 18]
        ws += [rng.randint(max(bot, -10 ** 18), min(top, 10 ** 18)) for _ in range(50)]
    seen = set()
    for w in ws:
        l, n = bv.score_limbs(w)
        assert l == score.limbs(w) and n == score.n_limbs(w), w
        assert all(-128 <= d <= 127 for d in l) and sum(d << (8 * a) for a, d in enumerate(l[:n])) == w
        seen.add(n)
    assert seen == set(range(1, 9)) and bv.score_limbs(10 ** 18)[1] == 8 and bv.score_limbs(-10 ** 18)[1] == 8


def test_decimal_text(bv):
    cases = {0: b"0", 1: b"0.000000000001", -1: b"-0.000000000001", 10 ** 12: b"1", -10 ** 12: b"-1", 5 * 10 ** 11: b"0.5",
             15 * 10 ** 11: b"1.5", 10 ** 12 + 10: b"1.00000000001", -(10 ** 13) - 100: b"-10.0000000001",
             300000 * 10 ** 18: b"300000000000", (1 << 64) * 10 ** 12 + 1: b"18446744073709551616.000000000001",
             -(1 << 100) + 7: None, (1 << 127) - 1: None, -(1 << 127): None}
    rng = random.Random(3)
    for _ in range(300):
        cases[rng.randint(-(1 << rng.randint(1, 127)), 1 << rng.randint(1, 127))] = None
    for t, text in cases.items():
        got = bv.score_decimal(t)
        assert got == score.decimal(t).encode() and (text is None or got == text), t
        assert not got.endswith(b"0") or b"." not in got
        assert Fraction(got.decode()) * 10 ** 12 == t


# ---- the file

GOOD = b"#locus\tPGS1\tPC one\r\n\r\nchr1:100:A:T\t1.5\t-2e-3\nchr2:5:G:+ACG\t0\t.25\n\nchrX:7:C:-3\t-1e6\t1E6\n"


def test_file_rules(bv):
    t = bv.ScoreTable(text=GOOD)
    names, entries = score.parse_file(GOOD)
    assert t.names == names == [b"PGS1", b"PC one"] and (t.n, t.n_columns, t.n_limbs) == (3, 2, 8)
    w = t.weights
    for loc, ws in entries:
        row = w[t.find(loc)]
        assert [sum(int(d) << (8 * a) for a, d in enumerate(row[c * 8:c * 8 + 8])) for c in range(2)] == ws and row[-1] == 1
    assert t.find(b"chr1:100:A:T\r") == -1 and t.find(b"chr1:100:A") == -1
    t.close()
    t = bv.ScoreTable(text=b"a\t1\t2\t3\nb\t-4\t5\t127")  # no header, no final newline, one limb
    assert t.names == [b"SCORE1", b"SCORE2", b"SCORE3"] == score.parse_file(b"a\t1\t2\t3\nb\t-4\t5\t127")[0]
    t.close()
    t = bv.ScoreTable(text=b"a\t1e-12\t0\n")
    assert (t.n_limbs, t.weights.tolist()) == (1, [[1, 0, 1]])
    t.close()
    t = bv.ScoreTable(text=b"\n#locus\tA\n\n")  # a header alone: nothing matches
    assert (t.n, t.n_columns, t.capacity, t.find(b"a")) == (0, 1, 16, -1) and score.parse_file(b"\n#locus\tA\n\n") == ([b"A"], [])
    t.close()
    wide = b"x\t" + b"\t".join([b"1"] * 64) + b"\n"
    t = bv.ScoreTable(text=wide)
    assert t.n_columns == 64
    t.close()


BAD_FILES = [(b"", 0), (b"\n\r\n\n", 0), (b"a\t1\n#locus\tb\n", 2), (b"#locus\tA\n#x\t1\n", 2), (b"a\t1\n\nb\t1\t2\n", 3), (b"a\t1\t2\nb\t1\n", 2),
             (b"a\n", 1), (b"#locus\n", 1), (b"x\t" + b"\t".join([b"1"] * 65) + b"\n", 1), (b"#locus\tA\tA\n", 1), (b"#locus\tA\t\n", 1),
             (b"#loci\tA\n", 1), (b"a\t1\n\t2\n", 2), (b"a\t1\nb\t2\na\t1\n", 3), (b"a\t1\nb\tnan\n", 2), (b"a\t1\nb\t1e7\n", 2),
             (b"a\t1\nb\t 1\n", 2), (b"a\t1\nb\t\n", 2), (b"a\t1\r\r\n", 1)]


@pytest.mark.parametrize("text,line", BAD_FILES)
def test_file_errors_name_their_line(bv, text, line):
    with pytest.raises(score.ScoreFileError) as ref:
        score.parse_file(text)
    assert ref.value.line == line
    with pytest.raises(bv.BvcfError) as ei:
        bv.ScoreTable(text=text)
    assert ei.value.rc == bv.E_ARG
    assert ("line %d: " % line in str(ei.value)) if line else ("line " not in str(ei.value)), str(ei.value)


def test_lookup_against_the_reference(bv):
    rng = random.Random(4)
    loci = [vl.snp_locus(p) for p in rng.sample(range(1, 100000), 3000)] + [b"chr2:5:G:+" + b"ACGT" * 200, b"c", b"chrUn_gl000220:1:A:-12"]
    ws = [[rng.randint(-10 ** 18, 10 ** 18), rng.randint(-5, 5)] for _ in loci]
    t = bv.ScoreTable(loci, ws)
    e = t.entries
    assert t.capacity == bv.variant_table_capacity(len(loci)) == len(e) and int((e["len"] != 0).sum()) == len(loci)
    rows = t.weights
    for i, (loc, w) in enumerate(zip(loci, ws)):
        r = t.find(loc)
        assert r == i, loc
        assert [sum(int(d) << (8 * a) for a, d in enumerate(rows[r][c * 8:c * 8 + 8])) for c in range(2)] == w
    for loc in vl.near_misses(loci[:200]) + [b"", b"chr1"]:
        assert t.find(loc) == (loci.index(loc) if loc in loci else -1)
    t.close()
    # two loci that agree in tag and home slot: the bytes decide
    a, b = (vl.snp_locus(p) for p in vl.collision_pair(bv))
    t = bv.ScoreTable([a], [[1]])
    assert t.find(a) == 0 and t.find(b) == -1
    t.close()
    t = bv.ScoreTable([a, b], [[1], [2]])
    assert (t.find(a), t.find(b)) == (0, 1)
    t.close()
    with pytest.raises(bv.BvcfError):
        bv.ScoreTable([a, a], [[1], [1]])
    with pytest.raises(bv.BvcfError):
        bv.ScoreTable([a], [[10 ** 18 + 1]])


# ---- the structs and the CLI

def test_header_and_exports(bv):
    with open(os.path.join(ROOT, "include", "bvcf.h")) as f:
        h = f.read()
    assert "#define BVCF_CONFIG_MORE_SCORE 8\n" in h and bv.CONFIG_MORE_SCORE == 8
    for name in ("bvcf_score_table_build", "bvcf_score_table_parse", "bvcf_score_table_free", "bvcf_score_table_find",
                 "bvcf_set_score_table", "bvcf_score", "bvcf_config_score_defaults"):
        assert name in bv.EXPORTS and hasattr(bv.lib, name)
    for name in ("bvcf_score_weight", "bvcf_score_limbs", "bvcf_score_decimal"):
        assert name in bv.PLAN_EXPORTS and hasattr(bv.lib, name)
    assert "bvcf_bench_score_kernels" in bv.BENCH_EXPORTS and hasattr(bv.lib, "bvcf_bench_score_kernels")
    assert bv.ABI_VERSION == 9 and bv.ABI_VERSION_SUBSET == 10


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    fields = ["score_path", "score_output_path", "score_report_path"]
    tf = [f for f, _ in bv.ScoreTableStruct._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\nint main(){'
                   'printf("%zu %zu %zu", sizeof(bvcf_config_grm), sizeof(bvcf_config_score), sizeof(bvcf_score_table));'
                   + "".join('printf(" %%zu", offsetof(bvcf_config_score, %s));' % f for f in fields)
                   + "".join('printf(" %%zu", offsetof(bvcf_score_table, %s));' % f for f in tf)
                   + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    G, T = bv.ConfigScore, bv.ScoreTableStruct
    assert out == [C.sizeof(bv.ConfigGrm), C.sizeof(G), C.sizeof(T)] + [getattr(G, f).offset for f in fields] + [getattr(T, f).offset for f in tf]
    assert G.score_path.offset == C.sizeof(bv.ConfigGrm) and G.grm.offset == 0


def test_older_defaults_write_what_they_wrote(bv):
    """each of the eight older *_defaults leaves everything behind its own struct alone; the new one fills the whole struct"""
    G = bv.ConfigScore
    older = ((bv.lib.bvcf_config_more_defaults, bv.ConfigMore.site_gate.offset, 0),
             (bv.lib.bvcf_config_gate_defaults, bv.ConfigMore.plink_prefix.offset, bv.CONFIG_MORE_GATE),
             (bv.lib.bvcf_config_plink_defaults, C.sizeof(bv.ConfigMore), bv.CONFIG_MORE_PLINK),
             (bv.lib.bvcf_config_trios_defaults, C.sizeof(bv.ConfigTrios), bv.CONFIG_MORE_TRIOS),
             (bv.lib.bvcf_config_ld_defaults, C.sizeof(bv.ConfigLd), bv.CONFIG_MORE_LD),
             (bv.lib.bvcf_config_variants_defaults, C.sizeof(bv.ConfigVariants), bv.CONFIG_MORE_VARIANTS),
             (bv.lib.bvcf_config_regions_defaults, C.sizeof(bv.ConfigRegions), bv.CONFIG_MORE_REGIONS),
             (bv.lib.bvcf_config_grm_defaults, C.sizeof(bv.ConfigGrm), bv.CONFIG_MORE_GRM))
    for fn, first_untouched, marker in older:
        g = G()
        C.memset(C.byref(g), 0xFF, C.sizeof(g))
        fn(C.byref(g))
        assert bytes(g)[first_untouched:] == b"\xff" * (C.sizeof(g) - first_untouched), fn
        base = g.grm.regions.variants.ld.trios.more.base
        assert base.reserved[0] == bv.CONFIG_MORE and base.reserved[1] == marker
    v = bv.ConfigGrm()
    bv.lib.bvcf_config_grm_defaults(C.byref(v))
    g = G()
    C.memset(C.byref(g), 0xFF, C.sizeof(g))
    bv.lib.bvcf_config_score_defaults(C.byref(g))
    assert g.grm.regions.variants.ld.trios.more.base.reserved[1] == bv.CONFIG_MORE_SCORE
    assert [g.score_path, g.score_output_path, g.score_report_path, g.grm.grm_prefix] == [None] * 4
    g.grm.regions.variants.ld.trios.more.base.reserved[1] = bv.CONFIG_MORE_GRM  # but for the marker, its head is what the older one makes
    assert bytes(g)[:C.sizeof(v)] == bytes(v)


def test_config_markers(bv):
    assert list(bv.make_config({"grm": "/x"}).reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_GRM]
    c = bv.make_config({"score": "/w", "scoreOutput": "/o", "minMac": 3, "excludeVariants": "/l"})
    assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_SCORE]
    g = C.cast(C.byref(c), C.POINTER(bv.ConfigScore)).contents
    assert (g.score_path, g.score_output_path, g.score_report_path, g.grm.grm_prefix) == (b"/w", b"/o", None, None)
    assert g.grm.regions.variants.exclude_variants_path == b"/l" and g.grm.regions.variants.ld.trios.more.site_gate.min_mac == 3


def cli(args, stdin_bytes=b""):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=60)


@pytest.mark.parametrize("flag", ["score", "scoreOutput", "scoreReport"])
def test_cli_flag_without_a_value(flag):
    p = cli(["--" + flag])
    assert p.returncode == 2 and p.stdout == b""
    assert p.stderr == ("flag needs an argument: -%s\n" % flag).encode()
    p = cli(["--%s=" % flag])
    assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1


@pytest.mark.parametrize("args", [["--score", "w"], ["--scoreOutput", "o"], ["--scoreReport", "r"], ["--scoreReport", "r", "--score", "w"]])
def test_cli_flags_come_together(args):
    p = cli(args, vl.rows_vcf(5))
    assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1


def test_cli_unreadable_and_unwritable(tmp_path):
    """one message and exit code 1, before the input is looked at or a device asked for"""
    w = tmp_path / "w.tsv"
    w.write_bytes(GOOD)
    bad = tmp_path / "no_such_dir" / "x"
    p = cli(["--score", str(bad), "--scoreOutput", str(tmp_path / "o")], vl.rows_vcf(5))
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.count(b"\n") == 1 and str(bad).encode() in p.stderr and b"No such file" in p.stderr
    for extra in (["--scoreOutput", str(bad)], ["--scoreOutput", str(tmp_path / "o"), "--scoreReport", str(bad)]):
        p = cli(["--score", str(w)] + extra, vl.rows_vcf(5))
        assert p.returncode == 1 and p.stdout == b""
        assert p.stderr.count(b"\n") == 1 and str(bad).encode() in p.stderr


@pytest.mark.parametrize("text,line", [c for c in BAD_FILES if c[1]][:8])
def test_cli_bad_score_file(text, line, tmp_path):
    w = tmp_path / "bad.tsv"
    w.write_bytes(text)
    p = cli(["--score", str(w), "--scoreOutput", str(tmp_path / "o")], vl.rows_vcf(5))
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.count(b"\n") == 1
    assert str(w).encode() in p.stderr and (b"line %d:" % line) in p.stderr


# ---- the GPU tests' inputs, with the oracle alone

def coverage(vcf, text, cfg=None):
    """what the rows of an input do against a score file: (matched rows with many carriers, matched rows with few, matched
    rows with a missing call, unmatched rows, columns without a non-zero weight)"""
    rc, body, _, _ = orc.run(vcf, cfg or {})
    assert rc == 0
    names, entries = score.parse_file(text)
    table = dict(entries)
    H, O, M = pt.matrices(body, pt.sample_names(vcf), cfg)
    loci = vl.loci_of(body)
    hit = np.array([x in table for x in loci], dtype=bool)
    car = H + O + M
    # a short class list holds at most 15 map bytes of 4 samples: a row with 16 carriers spread over 16 bytes cannot be one
    nbytes = np.array([len({i // 4 for i in np.flatnonzero(r)}) for r in car])
    dense, short = int((hit & (nbytes > 15)).sum()), int((hit & (nbytes <= 15)).sum())
    miss = int((hit & (M.sum(axis=1) > 0)).sum())
    zero_cols = [c for c in range(len(names)) if not any(ws[c] for _, ws in entries)]
    return dense, short, miss, int((~hit).sum()), zero_cols


def test_inputs_reach_every_case():
    for seed, *_ in pt.FUZZ:
        cfg = {"allow": ""} if seed % 2 else {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",", "emptyField": "NA"}
        vcf = pt.fuzz_vcf(seed)
        loci = vl.loci_of(orc.run(vcf, cfg)[1])
        text = score.file_text(score.entries_for(loci, 3, seed, big=bool(seed & 2), frac=0.6, extra=[b"chr9:1:A:T"]))
        dense, short, miss, unmatched, zero_cols = coverage(vcf, text, cfg)
        assert dense + short > 50 and miss > 0 and unmatched > 0 and not zero_cols, (seed, dense, short, miss, unmatched)
        # (the fuzz rows are common variants; a narrow cohort's rows always fit a short list: rare_vcf below has both forms)
        assert dense > 0 or len(pt.sample_names(vcf)) < 300, (seed, dense, short)
    vcf = pt.rare_vcf(300)
    loci = vl.loci_of(orc.run(vcf)[1])
    text = score.file_text(score.entries_for(loci, 4, 610, big=True, frac=0.7))
    dense, short, miss, unmatched, zero_cols = coverage(vcf, text)
    assert dense > 20 and short > 50 and miss > 0 and unmatched > 20 and not zero_cols
    # the short list at its limit is matched, with missing entries
    vcf = pt.short_list_limit_vcf()
    loci = vl.loci_of(orc.run(vcf)[1])
    dense, short, miss, unmatched, zero_cols = coverage(vcf, score.file_text(score.entries_for(loci, 2, 620, big=True)))
    assert dense >= 1 and short >= 15 and miss >= 3
    # the column of zeros is one, beside columns that are not
    vcf = pt.rare_vcf(129)
    loci = vl.loci_of(orc.run(vcf)[1])
    assert coverage(vcf, score.file_text(score.entries_for(loci, 3, 600, zero_column=1)))[4] == [1]
    # eight limbs beside one
    big = score.entries_for(loci, 2, 1, big=True)
    assert max(score.n_limbs(w) for _, ws in big for w in ws) == 8 and min(score.n_limbs(w) for _, ws in big for w in ws) == 1
    assert max(score.n_limbs(w) for _, ws in score.entries_for(loci, 2, 1) for w in ws) == 1
    assert 2 * score.FLUSH_ROWS * score.MAX_W >= 1 << 64


# ---- the shared header under sanitizers

def test_arithmetic_header_alone_under_sanitizers(tmp_path):
    """bvcf_score_q.h in a program of its own: every seeded weight text against Python's exact definition, the limbs, the
    128-bit adds across carries, the decimal text beyond 64 bits"""
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present: sanitized programs run on the build machine")
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "score_check")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "score_check.cpp"),
                           "-o", exe], timeout=120)
    texts = [t for t in seeded_texts(3000, seed=5) + [w for w, _ in WORKED] + REFUSED_BIG + REFUSED_BAD + other_texts() if b"\n" not in t]
    (tmp_path / "w.txt").write_bytes(b"".join(t + b"\n" for t in texts))
    p = subprocess.run([exe, str(tmp_path / "w.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.endswith("score_q ok\n"), out[-2000:]
    assert "ERROR" not in out and "runtime error" not in out, out[-2000:]
    lines = out.split("\n")[:-2]
    want = []
    for t in texts:
        try:
            w, rc = score.weight(t), 0
        except ValueError:
            w, rc = 0, -1
        except OverflowError:
            w, rc = 0, -2
        want.append(" ".join(str(x) for x in [rc, w] + score.limbs(w) + [score.n_limbs(w)]))
    one = score.ONE
    for t in (0, 1, -1, one, -one, one // 2, 15 * one // 10, -(1 << 100) + 7, (1 << 64) * one, 300000 * score.MAX_W, (1 << 127) - 1, -(1 << 127)):
        want.append(score.decimal(t))
    assert lines == want
