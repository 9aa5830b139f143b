"""--minGQ / --minDP (bvcf_params.min_gq / min_dp): what can be checked without a device -- the ABI, the CLI flags, the
masker the GPU tests take their expected output from (gtmask.py), and that the mask bites on every input they use."""
import ctypes as C
import os
import subprocess

import pytest

import gtmask
import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def _cli(args):
    return subprocess.run([EXE] + args, input=b"", capture_output=True, timeout=60)


# ---- binding and ABI

def test_make_config_carries_the_thresholds(bv):
    c = bv.make_config({"minGQ": 20, "minDP": 8})
    assert (c.min_gq, c.min_dp) == (20, 8)
    d = bv.make_config()
    assert (d.min_gq, d.min_dp) == (0, 0)
    assert bv.ABI_VERSION == 9
    p = bv.Params()
    assert (p.min_gq, p.min_dp) == (0, 0)


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\n'
                   "int main(){printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n\","
                   "offsetof(bvcf_params, min_gq), offsetof(bvcf_params, min_dp), sizeof(((bvcf_params *)0)->min_gq), sizeof(bvcf_params),"
                   "offsetof(bvcf_config, min_gq), offsetof(bvcf_config, min_dp), sizeof(((bvcf_config *)0)->min_dp), sizeof(bvcf_config),"
                   "offsetof(bvcf_config, sample_stats_path), offsetof(bvcf_params, want_sample_stats));"
                   "bvcf_config c; bvcf_config_defaults(&c); printf(\"%u %u %d %u\\n\", c.min_gq, c.min_dp, BVCF_ABI_VERSION,"
                   "BVCF_MAX_THRESHOLD); return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include"),
                           "-L", os.path.join(ROOT, "bystro-vcf_amd"), "-lbvcf",
                           "-Wl,-rpath," + os.path.join(ROOT, "bystro-vcf_amd")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    p_gq, p_dp, p_sz, p_size, c_gq, c_dp, c_sz, c_size, c_ss, p_ss = out[:10]
    assert (p_gq, p_dp, p_sz) == (bv.Params.min_gq.offset, bv.Params.min_dp.offset, bv.Params.min_gq.size)
    assert (c_gq, c_dp, c_sz) == (bv.Config.min_gq.offset, bv.Config.min_dp.offset, bv.Config.min_dp.size)
    assert p_size == C.sizeof(bv.Params) and c_size == C.sizeof(bv.Config)
    # appended: behind the last field of ABI 8
    assert p_gq == p_ss + 4 and p_dp == p_gq + 4 and c_gq == c_ss + C.sizeof(C.c_char_p) and c_dp == c_gq + 4
    assert out[10:] == [0, 0, 9, gtmask.MAX_THRESHOLD]


# ---- the CLI flags

@pytest.mark.parametrize("flag", ["--minGQ", "--minDP", "-minGQ"])
def test_cli_flag_reaches_the_no_out_check(flag):
    p = _cli([flag, "20", "--noOut"])
    assert p.returncode == 1, p.stderr
    assert b"When specifying --noOut, must specify --dosageOutput" in p.stderr
    assert b"flag provided but not defined" not in p.stderr


@pytest.mark.parametrize("flag", ["minGQ", "minDP"])
@pytest.mark.parametrize("val", ["x", "-1", "1000000000", "", "1.5", "+3", "0x10", "12345678901234567890"])
def test_cli_rejects_invalid_values(flag, val):
    for args in (["--" + flag, val], ["--%s=%s" % (flag, val)]):
        p = _cli(args + ["--noOut"])
        assert p.returncode == 2, (args, p.stderr)
        assert ('invalid value "%s" for flag -%s' % (val, flag)).encode() in p.stderr


def test_cli_flag_needs_a_value():
    p = _cli(["--minGQ"])
    assert p.returncode == 2 and b"flag needs an argument: -minGQ" in p.stderr


def test_cli_accepts_the_range_ends():
    for val in ("0", "999999999", "007"):
        p = _cli(["--minDP", val, "--noOut"])
        assert p.returncode == 1 and b"must specify --dosageOutput" in p.stderr, (val, p.stderr)


# ---- the masker itself

def test_key_index():
    ki = gtmask.key_index
    assert ki(b"GT:DP:GQ", b"GQ") == 2 and ki(b"GT:DP:GQ", b"DP") == 1
    assert ki(b"GQ:GT:DP", b"GQ") is None          # position 0 is the genotype, never a key
    assert ki(b"GQ:GQ", b"GQ") == 1
    assert ki(b"GT:GQX:DP", b"GQ") is None         # GQX does not match
    assert ki(b"GT:XGQ", b"GQ") is None and ki(b"GT:gq", b"GQ") is None and ki(b"GT:G", b"GQ") is None
    assert ki(b"GT:GQ:AD:GQ", b"GQ") == 1          # the first of two wins
    assert ki(b"GT", b"GQ") is None and ki(b"", b"DP") is None
    assert ki(b"GT:AD:DP:GQ:PL", b"GQ") == 3


def _line(fmt, *fields):
    return b"\t".join([b"1", b"100", b".", b"A", b"C", b"50", b"PASS", b"."] + [fmt] + list(fields))


@pytest.mark.parametrize("value,masked", [
    (b"19", True), (b"20", False), (b"0", True), (b"007", True), (b"000000019", True), (b"020", False),
    (None, False),            # absent: trailing subfields dropped
    (b"", False),             # empty
    (b".", False),            # the VCF missing value
    (b"-3", False), (b"+3", False),   # a sign
    (b"12.5", False),         # a decimal point
    (b"1e2", False), (b"1E1", False),  # an exponent
    (b"0000000005", False), (b"1234567890", False),  # 10 or more digits
    (b"123456789", False),    # 9 digits: a number, and not below 20
    (b"5 ", False), (b" 5", False), (b"5,5", False),
])
def test_rule_3_one_clause_at_a_time(value, masked):
    field = b"0/1:33" + (b"" if value is None else b":" + value)
    got = gtmask.mask_line(_line(b"GT:DP:GQ", field, b"1/1:40:60"), 20, 0)
    want_field = (b"./." + field[3:]) if masked else field
    assert got == _line(b"GT:DP:GQ", want_field, b"1/1:40:60")


def test_masker_rules_4_and_5_and_what_stays():
    ln = _line(b"GT:DP:GQ", b"0/1:5:60", b"1:30:5", b"0/1/1:30:60", b"./.:3:3", b"0|1:9:19:7,8", b"1/1", b"")
    # both thresholds: either key masks; haploid and polyploid calls are replaced whole; the rest of the field stays
    assert gtmask.mask_line(ln, 20, 10) == _line(b"GT:DP:GQ", b"./.:5:60", b"./.:30:5", b"0/1/1:30:60", b"./.:3:3",
                                                 b"./.:9:19:7,8", b"1/1", b"")
    assert gtmask.mask_line(ln, 20, 0) == _line(b"GT:DP:GQ", b"0/1:5:60", b"./.:30:5", b"0/1/1:30:60", b"./.:3:3",
                                                b"./.:9:19:7,8", b"1/1", b"")
    assert gtmask.mask_line(ln, 0, 0) == ln
    # a FORMAT without the key masks nothing; sites-only and short lines are left alone
    assert gtmask.mask_line(_line(b"GT:DP", b"0/1:5:1"), 20, 0) == _line(b"GT:DP", b"0/1:5:1")
    short = b"1\t100\t.\tA\tC\t50\tPASS\t."
    assert gtmask.mask_line(short, 20, 10) == short
    # a value at the very end of the line and in the last sample
    assert gtmask.mask_line(_line(b"GT:GQ", b"0/0:50", b"0/1:2"), 20, 0) == _line(b"GT:GQ", b"0/0:50", b"./.:2")


def test_mask_vcf_keeps_header_and_crlf():
    hdr = b"##fileformat=VCFv4.2\r\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\r\n"
    vcf = hdr + _line(b"GT:GQ", b"0/1:3", b"0/1:2") + b"\r\n" + _line(b"GT:GQ", b"0/1:30", b"1/1:20") + b"\r\n"
    st = {}
    got = gtmask.mask_vcf(vcf, 20, 0, st)
    assert got == hdr + _line(b"GT:GQ", b"./.:3", b"./.:2") + b"\r\n" + _line(b"GT:GQ", b"0/1:30", b"1/1:20") + b"\r\n"
    assert st == {"valued": 4, "masked": 2}
    assert gtmask.mask_vcf(vcf, 0, 0) == vcf
    # T = 1 masks "0" only; T = 999999999 masks everything that is a number below it
    lf = vcf.replace(b"\r\n", b"\n")
    one = lf + _line(b"GT:GQ", b"0/1:0", b"0/1:1") + b"\n"
    assert gtmask.mask_vcf(one, 1, 0).endswith(_line(b"GT:GQ", b"./.:0", b"0/1:1") + b"\n")
    top = lf + _line(b"GT:GQ", b"0/1:999999998", b"0/1:999999999") + b"\n"
    assert gtmask.mask_vcf(top, 999999999, 0).endswith(_line(b"GT:GQ", b"./.:999999998", b"0/1:999999999") + b"\n")


# ---- the mask bites on every seeded input of the GPU tests (the oracle alone)

@pytest.mark.parametrize("name", list(gtmask.SEEDED))
def test_seeded_inputs_are_bitten(bv, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    rc, out_o, log_o, _ = orc.run(vcf, cfg)
    assert rc == 0
    hdr = bv.string_header(cfg).split("\t")
    for gq, dp in gtmask.thresholds_of(name):
        m, st = gtmask.masked(name, gq, dp)
        share = st["masked"] / max(st["valued"], 1)
        assert 0.05 <= share <= 0.60, (name, gq, dp, st)
        rc, out_m, log_m, _ = orc.run(m, cfg)
        assert rc == 0 and out_m != out_o
        assert log_m == log_o  # rule 6: the log reads the fixed columns only
        gone, changed = gtmask.row_changes(out_o, out_m, hdr)
        assert len(gone) >= 1, (name, gq, dp, "no row disappears")
        assert len(changed) >= 1, (name, gq, dp, "no row keeps its place with a changed list")


def test_crafted_shapes_reach_the_long_fields():
    """the crafted files hold sample fields past 64 and past 1 024 bytes in front of a GQ value (the LDS window and the
    walk in global memory behind it); the alignment file holds a masked value at every alignment mod 16 and masked values
    that straddle the 1 KiB chunk boundary of their line's sample region (chunks start at the dword at or before the
    region's first byte)"""
    longest = 0
    n_long = 0
    for name in ("crafted37", "crafted130"):
        for ln in gtmask.seeded(name).split(b"\n"):
            cols = ln.split(b"\t")
            if len(cols) > 9 and gtmask.key_index(cols[8], b"GQ") is not None:
                lens = [len(f) for f in cols[9:]]
                longest = max(longest, max(lens))
                n_long += sum(1 for x in lens if x > 64)
    assert longest > 1024 and n_long > 20, (longest, n_long)
    for name, eol in (("alignment", 1), ("alignment_crlf", 2)):
        vcf = gtmask.seeded(name)
        body_at = vcf.index(b"\n", vcf.index(b"#CHROM")) + 1
        seen, value_on_boundary, field_over_boundary, off = set(), 0, 0, body_at
        for ln in vcf[body_at:].split(b"\n")[:-1]:
            cols = ln.split(b"\t")
            s_begin = off - body_at + sum(len(c) + 1 for c in cols[:9])  # offset in the block the device sees
            lb = s_begin & ~3
            at = s_begin
            for f in cols[9:]:
                f = f.rstrip(b"\r")
                if f.endswith(b":5"):  # masked by --minGQ 20; its value is the last byte
                    v = at + len(f) - 1
                    seen.add(v % 16)
                    # the value is the first byte of a chunk (its ':' the last of the one before), or the field starts in
                    # one chunk and its value lies in the next
                    value_on_boundary += (v - lb) % 1024 == 0
                    field_over_boundary += (at - lb) // 1024 != (v - lb) // 1024
                at += len(f) + 1
            off += len(ln) + 1
        assert seen == set(range(16)), name
        assert value_on_boundary >= 1 and field_over_boundary >= 5, (name, value_on_boundary, field_over_boundary)


@pytest.mark.parametrize("name", ["fuzz17", "fuzz70crlf", "fuzz300", "crafted37", "crafted5crlf", "alignment"])
def test_masked_dosage_rows_hold_missing_calls(name):
    """the inputs of the GPU dosage test: the oracle's rows of the masked bytes carry -1"""
    for gq, dp in gtmask.thresholds_of(name):
        want = [d for _, d in orc.run_dosage(gtmask.masked(name, gq, dp)[0], gtmask.SEEDED[name][1])]
        assert any(-1 in w for w in want)
