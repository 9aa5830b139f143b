"""The site gate (--minMaf / --maxMaf / --minMac / --maxMissing / --hwe), the parts that need no GPU: the exported per-row
code against the references of sitegate.py, the ABI's layout, the CLI's argument errors, and -- with the oracle alone --
that the inputs and thresholds of the GPU tests reach what those tests are about."""
import ctypes as C
import gzip
import os
import re
import subprocess
from fractions import Fraction

import pytest

import oracle_lib as orc
import pairtable as pt
import sitegate as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")
SIZES = [63, 64, 65, 300, 1000, 2504, 3000]  # the seeded triples of the exported code: 40 per size (and the corners)


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def worst(pairs):
    """(largest relative error, its triple) over (triple, got, want); an AssertionError for a value outside sg.close"""
    top = (0.0, ())
    for tr, got, want in pairs:
        assert sg.close(got, want), (tr, got, want)
        if want > sg.HWE_TINY:
            top = max(top, (abs(got - want) / want, tr))
    return top


def test_rational_reference_by_hand():
    # 2 het among 3: r = 2, support {0, 2}; w(0) = 3!/(1! 0! 2!) = 3, w(2) = 3! 4/(0! 2! 1!) = 12
    assert sg.weights_exact(2, 0, 1) == [3, 12]
    assert sg.hwe_exact_rational(2, 0, 1) == 1 and sg.hwe_exact_rational(0, 1, 2) == Fraction(3, 15)
    # Wigginton et al.'s own example (their Table: 100 individuals, 21 copies of the rarer allele)
    assert abs(float(sg.hwe_exact_rational(57, 14, 50)) - 0.842279756570793) < 1e-12
    # a tie is on the side of the observed term: with one het among two calls w(1) is the only term
    assert sg.hwe_exact_rational(1, 0, 1) == 1


def test_exported_hwe_on_every_small_triple(bv):
    tr = sg.small_triples(12)
    assert len(tr) == 455
    want = [float(sg.hwe_exact_rational(*t)) for t in tr]
    err, at = worst((t, bv.hwe_exact(*t), w) for t, w in zip(tr, want))
    print("bvcf_hwe_exact, n <= 12: worst relative error %.2e at %s" % (err, at))
    err, at = worst((t, sg.hwe_p(*t), w) for t, w in zip(tr, want))
    print("hwe_p, n <= 12: worst relative error %.2e at %s" % (err, at))


@pytest.mark.parametrize("n", SIZES)
def test_exported_hwe_on_seeded_triples(bv, n):
    tr = sg.seeded_triples(n, 40, 1)
    want = [float(sg.hwe_exact_rational(*t)) for t in tr]
    err, at = worst((t, bv.hwe_exact(*t), w) for t, w in zip(tr, want))
    print("bvcf_hwe_exact, n = %d: worst relative error %.2e at %s" % (n, err, at))
    err, at = worst((t, sg.hwe_p(*t), w) for t, w in zip(tr, want))
    print("hwe_p, n = %d: worst relative error %.2e at %s" % (n, err, at))
    assert any(w < 1e-6 for w in want) and any(w > 0.5 for w in want)


def test_verdict_boundaries(bv):
    """a row at a threshold stays: maf == F passes --minMaf F and --maxMaf F, n_miss / S == F passes --maxMissing F"""
    S = 200
    counts = (40, 400, 30, 5, 0)  # maf 0.1
    f = 40.0 / 400.0
    for cr in ({"minMaf": f}, {"maxMaf": f}, {"minMaf": f, "maxMaf": f}, {"minMac": 40}):
        assert bv.site_gate_verdict(cr, S, counts) == 0 == sg.verdict(cr, S, counts), cr
    above, below = float.fromhex("0x1.999999999999bp-4"), float.fromhex("0x1.9999999999999p-4")  # the neighbours of 0.1
    assert below < f < above
    assert bv.site_gate_verdict({"minMaf": above}, S, counts) == bv.GATE_MIN_MAF
    assert bv.site_gate_verdict({"maxMaf": below}, S, counts) == bv.GATE_MAX_MAF
    assert bv.site_gate_verdict({"minMac": 41}, S, counts) == bv.GATE_MIN_MAC
    miss = (40, 340, 30, 5, 30)  # 30 of 200 missing
    assert bv.site_gate_verdict({"maxMissing": 30.0 / 200.0}, S, miss) == 0
    assert bv.site_gate_verdict({"maxMissing": 29.0 / 200.0}, S, miss) == bv.GATE_MAX_MISSING
    # the minor allele is the rarer one: ac above an / 2 counts an - ac
    assert bv.site_gate_verdict({"minMac": 11}, S, (390, 400, 10, 190, 0)) == bv.GATE_MIN_MAC
    assert bv.site_gate_verdict({"minMac": 10}, S, (390, 400, 10, 190, 0)) == 0
    # every criterion a row fails is named, the exact test among them
    every = {"minMaf": 0.2, "maxMaf": 0.05, "minMac": 50, "maxMissing": 0.1, "hwe": 0.9}
    assert bv.site_gate_verdict(every, S, (40, 340, 0, 20, 30)) == 31 == sg.verdict(every, S, (40, 340, 0, 20, 30))
    assert bv.site_gate_verdict({}, S, counts) == 0  # the neutral gate


@pytest.mark.parametrize("name", ["rare300", "sweep", "fuzz13", "tile130", "one"])
def test_verdict_against_the_reference_on_file_rows(bv, name):
    """bvcf_site_gate_verdict on the counts of every TSV row of an input, each criterion alone and all together"""
    vcf = sg.case_input(name)
    rc, body, _, _ = orc.run(vcf)
    assert rc == 0
    S = len(pt.sample_names(vcf))
    rows = [sg.row_counts(r.split(b"\t")) for r in body.split(b"\n") if r]
    sets = sg.CASES[name]
    for cr in sets + [c for s in sets for c in sg.singles(s)]:
        got = [bv.site_gate_verdict(cr, S, c) for c in rows]
        assert got == [sg.verdict(cr, S, c) for c in rows], cr


def test_set_site_gate_range_checks(bv):
    for bad in ({"minMaf": 0.51}, {"minMaf": -0.1}, {"maxMaf": 1.5}, {"maxMissing": -1e-9}, {"hwe": 1.0001}, {"hwe": float("nan")},
                {"minMaf": float("nan")}, {"minMac": 1000000000}, {"maxMissing": float("inf")}):
        assert bv.site_gate_verdict(bad, 10, (1, 20, 1, 0, 0)) == -1, bad
    g = bv.make_site_gate()
    g.size = 8
    assert bv.site_gate_verdict(g, 10, (1, 20, 1, 0, 0)) == -1


def test_header_binding_and_library_agree(bv):
    with open(os.path.join(ROOT, "include", "bvcf.h")) as f:
        h = f.read()
    assert re.search(r"int bvcf_set_site_gate\(bvcf_ctx \*ctx, const bvcf_site_gate \*g\);", h)
    assert re.search(r"void bvcf_site_gate_count\(const bvcf_result \*r, uint64_t out\[7\]\);", h)
    for name, bit in (("MIN_MAF", 1), ("MAX_MAF", 2), ("MIN_MAC", 4), ("MAX_MISSING", 8), ("HWE", 16)):
        assert "#define BVCF_GATE_%s %du\n" % (name, bit) in h and getattr(bv, "GATE_" + name) == bit
    for name in ("bvcf_set_site_gate", "bvcf_site_gate_count", "bvcf_site_gate_defaults", "bvcf_config_gate_defaults"):
        assert name in bv.EXPORTS and hasattr(bv.lib, name)
    for name in ("bvcf_site_gate_verdict", "bvcf_hwe_exact", "bvcf_hwe_inline_terms"):
        assert name in bv.PLAN_EXPORTS and hasattr(bv.lib, name)
    for name in ("bvcf_bench_hwe", "bvcf_bench_gate_kernels"):
        assert name in bv.BENCH_EXPORTS and hasattr(bv.lib, name)
    assert bv.SITE_GATE_REPORT == sg.REPORT
    assert bv.ABI_VERSION == 9 and bv.ABI_VERSION_SUBSET == 10


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    fields = ["size", "min_mac", "min_maf", "max_maf", "max_missing", "hwe_p"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu", sizeof(bvcf_config), sizeof(bvcf_config_more), sizeof(bvcf_site_gate),'
                   "offsetof(bvcf_config_more, pair_stats_path), offsetof(bvcf_config_more, site_gate),"
                   "offsetof(bvcf_config_more, site_filter_path), sizeof(bvcf_allele));"
                   + "".join('printf(" %%zu", offsetof(bvcf_site_gate, %s));' % f for f in fields)
                   + 'printf(" %zu\\n", offsetof(bvcf_allele, pad)); return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M, G = bv.ConfigMore, bv.SiteGate
    assert out == [C.sizeof(bv.Config), C.sizeof(M), C.sizeof(G), M.pair_stats_path.offset, M.site_gate.offset,
                   M.site_filter_path.offset, 64] + [getattr(G, f).offset for f in fields] + [54]
    assert C.sizeof(G) == 40 and M.pair_stats_path.offset == C.sizeof(bv.Config)


def test_config_markers(bv):
    """a config without gate keys is what it was; the gate's fields count only with the second marker"""
    m = bv.ConfigMore()
    C.memset(C.byref(m), 0xFF, C.sizeof(m))
    bv.lib.bvcf_config_more_defaults(C.byref(m))
    # (a caller built when pair_stats_path was the last field owns no more: nothing behind it is written)
    assert m.base.reserved[0] == bv.CONFIG_MORE and m.base.reserved[1] == 0 and m.pair_stats_path is None
    assert bytes(m)[M_OFF(bv):] == b"\xff" * (C.sizeof(m) - M_OFF(bv))
    bv.lib.bvcf_config_gate_defaults(C.byref(m))
    assert (m.base.reserved[0], m.base.reserved[1]) == (bv.CONFIG_MORE, bv.CONFIG_MORE_GATE)
    g = m.site_gate
    assert (g.size, g.min_mac, g.min_maf, g.max_maf, g.max_missing, g.hwe_p) == (40, 0, 0.0, 1.0, 1.0, 0.0)
    assert m.site_filter_path is None and m.pair_stats_path is None
    assert list(bv.make_config({}).reserved) == [0, 0]
    assert list(bv.make_config({"relatedness": "/x"}).reserved) == [bv.CONFIG_MORE, 0]
    c = bv.make_config({"minMaf": 0.05, "hwe": 1e-6, "siteFilterReport": "/x/y"})
    assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_GATE]
    more = C.cast(C.byref(c), C.POINTER(bv.ConfigMore)).contents
    assert (more.site_gate.min_maf, more.site_gate.max_maf, more.site_gate.hwe_p) == (0.05, 1.0, 1e-6)
    assert more.site_filter_path == b"/x/y" and more.pair_stats_path is None


def M_OFF(bv):
    return bv.ConfigMore.site_gate.offset


def cli(args, stdin_bytes=b""):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=60)


@pytest.mark.parametrize("flag,val", [("minMaf", "0.6"), ("minMaf", "-0.1"), ("minMaf", "+0.1"), ("minMaf", " 0.1"), ("minMaf", "0.1x"),
                                      ("minMaf", ""), ("minMaf", "nan"), ("maxMaf", "1.5"), ("maxMaf", "inf"), ("maxMaf", "1e400"),
                                      ("maxMissing", "0x1p-2"), ("maxMissing", "1.0000001"), ("hwe", "2"), ("hwe", "1e-6 "),
                                      ("hwe", "0,05"), ("minMac", "1000000000"), ("minMac", "-1"), ("minMac", "2.5")])
def test_cli_refuses_bad_values(flag, val):
    for args in (["--" + flag, val], ["--%s=%s" % (flag, val)]):
        p = cli(args)
        assert p.returncode == 2, (args, p.stderr)
        assert p.stderr.count(b"\n") == 1 and ('invalid value "%s" for flag -%s: want' % (val, flag)).encode() in p.stderr, p.stderr
        assert p.stdout == b""


@pytest.mark.parametrize("flag", ["minMaf", "maxMaf", "minMac", "maxMissing", "hwe", "siteFilterReport"])
def test_cli_flag_without_a_value(flag):
    p = cli(["--" + flag])
    assert p.returncode == 2 and ("flag needs an argument: -%s" % flag).encode() in p.stderr


# ---- the input conditions of tests/test_gpu_site_gate.py, with the oracle alone

def oracle_rows(vcf):
    rc, body, _, _ = orc.run(vcf)
    assert rc == 0
    S = len(pt.sample_names(vcf))
    return body, S


def conditions(name, vcf, sets):
    body, S = oracle_rows(vcf)
    n_rows = body.count(b"\n")
    p_values = sg.row_p_values(body, S)
    for cr in sets:
        _, counts, _ = sg.gate(body, S, cr)
        assert counts[0] == n_rows
        for q, key in enumerate(sg.REPORT[2:]):
            if key not in cr:
                assert counts[2 + q] == 0
            elif n_rows > 1:
                assert 0 < counts[2 + q] < n_rows, "%s: %s = %r fails %d of %d rows" % (name, key, cr[key], counts[2 + q], n_rows)
        if "hwe" in cr:
            near = [p for p in p_values if abs(p - cr["hwe"]) <= 1e-6 * cr["hwe"]]
            assert not near, (name, cr["hwe"], near)
    return body, S


@pytest.mark.parametrize("name", sorted(sg.CASES))
def test_inputs_keep_and_drop_under_every_criterion(name):
    body, S = conditions(name, sg.case_input(name), sg.CASES[name])
    if name == "tile1":  # one row: one set keeps it, the other fails it under all five criteria
        assert [sg.gate(body, S, cr)[1][1:] for cr in sg.CASES[name]] == [[1, 0, 0, 0, 0, 0], [0, 1, 1, 1, 1, 1]]
    if name in ("rare300", "short", "sweep", "fuzz13", "cohort"):  # rows on both sides of the inline / wave bound
        terms = [len(sg.support(*sg.triple(S, *sg.row_counts(r.split(b"\t"))[2:]))[2]) for r in body.split(b"\n") if r]
        assert min(terms) <= 32 < max(terms), (min(terms), max(terms))


def test_golden_slice_keeps_and_drops():
    with gzip.open(GOLDEN_GZ, "rb") as f:
        vcf = f.read()
    body, S = conditions("golden", vcf, [sg.GOLDEN])
    assert S == 2504 and max(len(sg.support(*sg.triple(S, *sg.row_counts(r.split(b"\t"))[2:]))[2])
                             for r in body.split(b"\n") if r) == 1253


def golden_triples():
    with gzip.open(GOLDEN_GZ, "rb") as f:
        body, S = oracle_rows(f.read())
    return sorted({sg.triple(S, *sg.row_counts(r.split(b"\t"))[2:]) for r in body.split(b"\n") if r})


def test_near_tie_is_the_margin_test():
    lim = Fraction(1, 10 ** 9)
    for t in sg.small_triples(12) + sg.seeded_triples(300, 40, 1):
        m = sg.tie_margin(*t)
        assert sg.near_tie(*t) == (m is not None and m <= lim), t
    # ratios 2 and 1/2 are far; a made-up pair of weights at the factor itself is near
    assert not sg.near_tie(2, 0, 1)
    wa = 10 ** 9
    assert wa * 1000000099 <= 1000000100 * 10 ** 9 <= wa * 1000000101


@pytest.mark.parametrize("which", ["cpu", "files", "device", "golden"])
def test_no_term_ratio_near_the_tie_factor(which):
    """no w(h) / w(a) of a tested triple within 1e-9 of 1 + 1e-7 unless it equals 1: the verdict on every term is the
    same in exact and in float arithmetic.  cpu: the triples of this file; files: every row of the file-level cases that
    are run with --hwe (the masked and the cut file among them); device: the triples tests/test_gpu_site_gate.py hands to
    bvcf_bench_hwe, up to sg.MARGIN_CHECK_MAX_N calls; golden: the distinct triples of the golden slice's rows"""
    if which == "cpu":
        triples = set(sg.small_triples(12))
        for n in SIZES:
            triples.update(sg.seeded_triples(n, 40, 1))
    elif which == "files":
        triples = set()
        for name in sg.CASES:
            if any("hwe" in cr for cr in sg.CASES[name]):
                body, S = oracle_rows(sg.case_input(name))
                triples.update(sg.triple(S, *sg.row_counts(r.split(b"\t"))[2:]) for r in body.split(b"\n") if r)
    elif which == "device":
        every = sg.all_device_triples()
        triples = [t for t in every if sum(t) <= sg.MARGIN_CHECK_MAX_N]
        # what is left out: the triples of 100 000 calls, whose yardstick is hwe_p
        assert {sum(t) for t in every if sum(t) > sg.MARGIN_CHECK_MAX_N} == {100000}
        assert len(triples) > 600 and any(sum(t) == 10000 for t in triples) and set(sg.SEGMENTS) <= set(triples)
    else:
        triples = golden_triples()
        assert len(triples) > 1000
    near = [t for t in sorted(triples) if sg.near_tie(*t)]
    assert not near, near[:5]


def test_device_bound_is_the_exported_one(bv):
    """the triples of the device test straddle the bound the library reports, which is the kernel's constant"""
    with open(os.path.join(ROOT, "bystro-vcf_amd", "csrc", "bvcf_sitegate.hip.h")) as f:
        m = re.search(r"constexpr uint32_t kHweInlineTerms = (\d+);", f.read())
    bound = bv.hwe_inline_terms()
    assert m and int(m.group(1)) == bound
    for n in sg.DEVICE_SIZES:
        terms = [len(sg.support(*t)[2]) for t in sg.device_triples(n)]
        assert min(terms) <= bound
        assert (max(terms) > bound) == (n >= 64) and (n != 63 or max(terms) == bound)
        if n >= 66:
            assert {bound - 1, bound, bound + 1, bound + 2} <= set(terms)


def test_sweep_input_spans_the_test():
    body, S = oracle_rows(sg.hwe_sweep_vcf())
    p = sg.row_p_values(body, S)
    rows = [sg.row_counts(r.split(b"\t")) for r in body.split(b"\n") if r]
    assert S == 300 and min(p) < 1e-30 and sum(x > 0.5 for x in p) > 20 and sum(1e-6 < x < 0.05 for x in p) > 10
    assert sum(c[4] > 60 for c in rows) > 20 and sum(c[4] == 0 for c in rows) > 20  # missing calls, and none
    # both kinds of departure: fewer and more heterozygotes than 2 n q (1 - q)
    dev = [c[2] - 2.0 * (S - c[4]) * (c[0] / c[1]) * (1 - c[0] / c[1]) for c, x in zip(rows, p) if x < 1e-6]
    assert min(dev) < -10 and max(dev) > 10
    vcf = sg.hwe_sweep_vcf()
    assert sum(1 for ln in vcf.split(b"\n") if b"\tC,G\t" in ln) == 9  # the multiallelic lines
