"""--keepSamples / --excludeSamples (bvcf_params.sample_keep): what can be checked without a device -- the ABI, the CLI
flags, the cutter the GPU tests take their expected output from (samplecut.py), and that the cut bites on every input
they use."""
import ctypes as C
import os
import subprocess

import pytest

import gtmask
import oracle_lib as orc
import samplecut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")

# the inputs whose tenth selection has to keep rows, drop rows and change lists (the alignment files keep all their rows
# under any selection and wide33000 is for shape coverage: the GPU tests use them for that only)
BITTEN = ["fuzz17", "fuzz70crlf", "fuzz300", "fuzz2600crlf", "crafted37", "crafted5crlf", "crafted130", "cohort", "stats300"]


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def _cli(args):
    return subprocess.run([EXE] + args, input=b"", capture_output=True, timeout=60)


# ---- binding and ABI

def test_binding_carries_the_selection(bv, tmp_path):
    assert bv.ABI_VERSION_SUBSET == 10  # the version that carries sample_keep; ABI 9 callers are still served
    c = bv.make_config({"keepSamples": str(tmp_path / "k"), "excludeSamples": str(tmp_path / "x")})
    assert c.keep_samples_path == str(tmp_path / "k").encode() and c.exclude_samples_path == str(tmp_path / "x").encode()
    d = bv.make_config()
    assert d.keep_samples_path is None and d.exclude_samples_path is None
    assert not bv.Params().sample_keep  # NULL: all samples


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\n'
                   "int main(){printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n\","
                   "offsetof(bvcf_params, sample_keep), sizeof(((bvcf_params *)0)->sample_keep), sizeof(bvcf_params),"
                   "offsetof(bvcf_config, keep_samples_path), offsetof(bvcf_config, exclude_samples_path),"
                   "sizeof(((bvcf_config *)0)->keep_samples_path), sizeof(bvcf_config),"
                   "offsetof(bvcf_params, min_dp), offsetof(bvcf_config, min_dp));"
                   "bvcf_config c; bvcf_config_defaults(&c); printf(\"%d %d %d\\n\", c.keep_samples_path == 0,"
                   "c.exclude_samples_path == 0, BVCF_ABI_VERSION_SUBSET); return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include"),
                           "-L", os.path.join(ROOT, "bystro-vcf_amd"), "-lbvcf",
                           "-Wl,-rpath," + os.path.join(ROOT, "bystro-vcf_amd")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    p_keep, p_sz, p_size, c_keep, c_excl, c_sz, c_size, p_dp, c_dp = out[:9]
    ptr = C.sizeof(C.c_void_p)
    assert (p_keep, p_sz) == (bv.Params.sample_keep.offset, bv.Params.sample_keep.size) and p_sz == ptr
    assert (c_keep, c_excl, c_sz) == (bv.Config.keep_samples_path.offset, bv.Config.exclude_samples_path.offset,
                                      bv.Config.keep_samples_path.size)
    assert p_size == C.sizeof(bv.Params) and c_size == C.sizeof(bv.Config)
    # appended: behind the last field of ABI 9 (a pointer, so at the next multiple of its size)
    assert (p_dp, c_dp) == (bv.Params.min_dp.offset, bv.Config.min_dp.offset)
    assert p_keep == (p_dp + 4 + ptr - 1) // ptr * ptr and p_size == p_keep + ptr
    assert c_keep == (c_dp + 4 + ptr - 1) // ptr * ptr and c_excl == c_keep + ptr and c_size == c_excl + ptr
    assert out[9:] == [1, 1, 10]


# ---- the CLI flags

@pytest.mark.parametrize("flag", ["--keepSamples", "--excludeSamples", "-keepSamples"])
def test_cli_flag_reaches_the_no_out_check(flag, tmp_path):
    for args in ([flag, str(tmp_path / "list")], ["%s=%s" % (flag, tmp_path / "list")]):
        p = _cli(args + ["--noOut"])
        assert p.returncode == 1, p.stderr
        assert b"When specifying --noOut, must specify --dosageOutput" in p.stderr
        assert b"flag provided but not defined" not in p.stderr


@pytest.mark.parametrize("flag", ["keepSamples", "excludeSamples"])
def test_cli_flag_needs_a_value(flag):
    p = _cli(["--" + flag])
    assert p.returncode == 2 and ("flag needs an argument: -" + flag).encode() in p.stderr
    p = _cli(["--%s=" % flag, "--noOut"])
    assert p.returncode == 2 and ("for flag -" + flag).encode() in p.stderr


def test_cli_rejects_both_flags(tmp_path):
    for args in (["--keepSamples", "a", "--excludeSamples", "b"], ["--excludeSamples=b", "-keepSamples=a"]):
        p = _cli(args + ["--noOut"])
        assert p.returncode == 2, p.stderr
        assert b"keepSamples" in p.stderr and b"excludeSamples" in p.stderr and b"both" in p.stderr


# ---- the cutter itself

HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\tC\tD\n"


def _line(*fields):
    return b"\t".join([b"1", b"100", b".", b"A", b"C", b"50", b"PASS", b".", b"GT"] + list(fields))


def test_cut_keeps_columns_in_header_order():
    vcf = HDR + _line(b"0/1", b"1/1", b"./.", b"0/0") + b"\n" + _line(b"0|0", b"0|1", b"1|0", b"1|1:7") + b"\n"
    got = samplecut.cut_vcf(vcf, [3, 1, 1])  # any order, duplicates harmless
    assert got == (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tB\tD\n" +
                   _line(b"1/1", b"0/0") + b"\n" + _line(b"0|1", b"1|1:7") + b"\n")
    assert samplecut.cut_vcf(vcf, range(4)) == vcf
    assert samplecut.sample_names(got) == [b"B", b"D"]


def test_cut_replaces_lines_of_another_field_count():
    short = _line(b"0/1", b"1/1", b"0/0")               # 12 fields: one too few
    long_ = _line(b"0/1", b"1/1", b"0/0", b"0/0", b"1/1")  # 14 fields: one too many
    sites = b"1\t300\t.\tG\tT\t50\tPASS\t."             # 8 fields
    tiny = b"1\t400"
    vcf = HDR + b"\n".join([short, long_, sites, tiny, _line(b"0/1", b"0/0", b"0/0", b"")]) + b"\n"
    got = samplecut.cut_vcf(vcf, [0, 3]).split(b"\n")
    first8 = b"\t".join(short.split(b"\t")[:8])
    assert got[2] == first8 and got[3] == first8 and got[4] == sites and got[5] == tiny
    assert got[6] == _line(b"0/1", b"")  # an empty trailing field stays one when the last column is kept ...
    assert samplecut.cut_vcf(vcf, [0, 1]).split(b"\n")[6] == _line(b"0/1", b"0/0")  # ... and goes with its column


def test_cut_keeps_crlf():
    vcf = HDR.replace(b"\n", b"\r\n") + _line(b"0/1", b"1/1", b"./.", b"0/0") + b"\r\n" + b"1\t2\r\n"
    got = samplecut.cut_vcf(vcf, [2])
    assert got == (b"##fileformat=VCFv4.2\r\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tC\r\n" +
                   _line(b"./.") + b"\r\n" + b"1\t2\r\n")


def test_selections_have_their_shapes():
    for name in gtmask.SEEDED:
        ns = samplecut.n_samples(name)
        sel = {k: samplecut.selection(name, k) for k in samplecut.KINDS}
        for k, s in sel.items():
            assert list(s) == sorted(set(s)) and 0 <= s[0] and s[-1] < ns and len(s) >= 1, (name, k)
        assert len(sel["one"]) == 1 and len(sel["allbutone"]) == ns - 1 and sel["ends"] == (0, ns - 1)
        assert len(sel["half"]) == max(1, ns // 2) and len(sel["tenth"]) == max(1, (ns + 5) // 10)
        assert samplecut.selection(name, "tenth") is sel["tenth"]  # cached, and the same on every call
        assert sorted(sel["half"] + samplecut.complement(name, sel["half"])) == list(range(ns))
    # the wide input's selections reach past sample 32 768, and its words past the 1 024th
    assert samplecut.selection("wide33000", "tenth")[-1] >= 32768


# ---- the cut bites on the seeded inputs of the GPU tests (the oracle alone)

@pytest.mark.parametrize("name", BITTEN)
def test_seeded_inputs_are_bitten(bv, name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    rc, out_o, log_o, _ = orc.run(vcf, cfg)
    assert rc == 0
    hdr = bv.string_header(cfg).split("\t")
    rc, out_c, log_c, _ = orc.run(samplecut.cut(name, "tenth"), cfg)
    assert rc == 0
    n_o, n_c = out_o.count(b"\n"), out_c.count(b"\n")
    print(name, "TSV body lines: original", n_o, "tenth kept", n_c)
    assert n_c >= 1, "the cut run keeps no row"
    assert log_c == log_o  # the log reads the fixed columns only
    gone, changed = gtmask.row_changes(out_o, out_c, hdr)
    assert len(gone) >= 1 and n_c < n_o, (name, "no row disappears")
    assert len(changed) >= 1, (name, "no row keeps its place with a changed list")


@pytest.mark.parametrize("name", ["alignment", "alignment_crlf"])
def test_alignment_inputs_keep_their_log(name):
    vcf, cfg = gtmask.seeded(name), gtmask.SEEDED[name][1]
    for kind in ("half", "one"):
        rc, out_c, log_c, _ = orc.run(samplecut.cut(name, kind), cfg)
        assert rc == 0 and out_c.count(b"\n") >= 1 and log_c == orc.run(vcf, cfg)[2]


def test_cut_commutes_with_the_mask():
    """masking and cutting touch different things -- a kept field's genotype subfield, whole columns -- so either order
    gives the same bytes: what the composition test on the device relies on"""
    for name in ("crafted37", "fuzz70crlf"):
        vcf = gtmask.seeded(name)
        sel = samplecut.selection(name, "half")
        assert samplecut.cut_vcf(gtmask.mask_vcf(vcf, 20, 10), sel) == gtmask.mask_vcf(samplecut.cut_vcf(vcf, sel), 20, 10)


# ---- the run's fatal path: the list is read and matched before any device work

def test_run_buffer_list_errors(bv, tmp_path):
    vcf = gtmask.seeded("crafted5crlf")
    unknown = tmp_path / "unknown.list"
    unknown.write_bytes(b"S00001\r\nNOBODY\r\nNOONE\r\n")
    empty = tmp_path / "empty.list"
    empty.write_bytes(b"\n\r\n")
    everyone = samplecut.list_file(tmp_path / "all.list", vcf, range(5))
    for cfg, word in [({"keepSamples": str(unknown)}, '"NOBODY"'), ({"excludeSamples": str(unknown)}, '"NOBODY"'),
                      ({"keepSamples": str(empty)}, "nothing would be left"),
                      ({"excludeSamples": everyone}, "nothing would be left"),
                      ({"keepSamples": str(tmp_path / "missing.list")}, "missing.list"),
                      ({"excludeSamples": str(tmp_path)}, "read ")]:
        rc, out, log, _ = bv.run_buffer(vcf, cfg)
        assert rc == bv.E_FATAL and out == b"", (cfg, rc)
        assert word in log and "NOONE" not in log and log.count("\n") == 1, (cfg, log)
    rc, _, log, _ = bv.run_buffer(vcf, {"keepSamples": everyone, "excludeSamples": str(empty)})
    assert rc == bv.E_ARG and log.count("\n") == 1
    # a file without sample columns: a name is unknown
    sites = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n1\t100\t.\tA\tC\t50\tPASS\t.\n"
    rc, _, log, _ = bv.run_buffer(sites, {"keepSamples": everyone})
    assert rc == bv.E_FATAL and '"S00000"' in log
