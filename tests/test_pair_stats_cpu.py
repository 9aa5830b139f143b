"""--relatedness, the parts that need no GPU: the test inputs reach what the GPU tests are about (checked with the oracle
alone), the ABI declares the new calls, the CLI parses the flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
import pairtable as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def pair_facts(t):
    """over the pairs i < j: (pairs with hetHet > 0, with ibs0 > 0, with het1 or het2 below the het count, with den == 0)"""
    hh, oc, hm = (x.astype(np.int64) for x in t)
    iu = np.triu_indices(hh.shape[0], 1)
    d = np.diag(oc)
    ibs0 = (d[:, None] - oc) + (d[None, :] - oc.T)
    het1 = np.diag(hh)[:, None] - hm
    den = 4 * np.minimum(het1, het1.T)
    return int((hh[iu] > 0).sum()), int((ibs0[iu] > 0).sum()), int(((hm + hm.T)[iu] > 0).sum()), int((den[iu] == 0).sum())


@pytest.mark.parametrize("name", sorted(pt.seeded_inputs()))
def test_seeded_inputs_reach_every_term(name):
    t, text = pt.expected(orc.run, pt.seeded_inputs()[name])
    het_het, ibs0, het_cut, _ = pair_facts(t)
    assert het_het > 0 and ibs0 > 0 and het_cut > 0, (het_het, ibs0, het_cut)
    assert (t[0] == t[0].T).all() and not np.diag(t[2]).any()
    assert text.count(b"\n") == 1 + t.shape[1] * (t.shape[1] - 1) // 2


def test_crafted_inputs():
    t, text = pt.expected(orc.run, pt.never_het_vcf(), {"emptyField": "NA"})
    assert pair_facts(t)[3] == 8 and text.count(b"\tNA\n") == 8
    t, _ = pt.expected(orc.run, pt.half_missing_vcf())
    assert pt.derive(t, 0, 1)[2] == 30 and int(t[0][0, 0]) == 60
    for n_rows in pt.TILE_ROWS:
        assert orc.run(pt.tile_vcf(n_rows))[1].count(b"\n") == n_rows
    # the short list at its limit: rows of 15 and of 16 non-zero map bytes
    body = orc.run(pt.short_list_limit_vcf())[1]
    H, O, M = pt.matrices(body, pt.sample_names(pt.short_list_limit_vcf()))
    nz_bytes = ((H + O + M).reshape(H.shape[0], -1, 4).sum(axis=2) > 0).sum(axis=1)
    assert list(nz_bytes[:4]) == [15, 16, 15, 1]


def test_kinship_by_hand():
    """two samples, four rows: 0|1 0|1, 1|1 0|0, 0|1 ./., 0|1 1|1"""
    rows = [("0|1", "0|1"), ("1|1", "0|0"), ("0|1", "./."), ("0|1", "1|1")]
    vcf = (pt.vcfgen.header(2) + "".join(pt.snp_line(10 + k, list(g)) for k, g in enumerate(rows))).encode()
    t, text = pt.expected(orc.run, vcf)
    # hetHet 1; ibs0 1 (row 2); het1 = 3 - 1 (row 3 has the other missing) = 2; het2 = 1; num = 2 - 4 - 2 - 1 = -5; den = 4
    assert pt.derive(t, 0, 1) == (1, 1, 2, 1, -5, 4)
    assert text.split(b"\n")[1] == b"S00000\tS00001\t1\t1\t2\t1\t-0.75"


def test_header_binding_and_library_agree(bv):
    with open(os.path.join(ROOT, "include", "bvcf.h")) as f:
        h = f.read()
    assert re.search(r"int bvcf_enable_pair_stats\(bvcf_ctx \*ctx\);", h)
    assert re.search(r"int bvcf_pair_stats\(bvcf_ctx \*ctx, uint64_t \*out[^;]*, int reset\);", h)
    assert "#define BVCF_PAIR_MAX_SAMPLES 8192u" in h and bv.PAIR_MAX_SAMPLES == 8192
    for name in ("bvcf_enable_pair_stats", "bvcf_pair_stats"):
        assert name in bv.EXPORTS and hasattr(bv.lib, name)
    assert bv.PAIR_STATS_COLUMNS == pt.COLUMNS
    assert bv.string_header().split("\t") == pt.BASE_HEADER


def test_config_defaults_leave_the_path_null(bv):
    """bvcf_config keeps its size; the path lives behind it, in bvcf_config_more"""
    m = bv.ConfigMore()
    C.memset(C.byref(m), 0xFF, C.sizeof(m))
    bv.lib.bvcf_config_more_defaults(C.byref(m))
    assert m.pair_stats_path is None and m.base.reserved[0] == bv.CONFIG_MORE
    assert m.base.empty_field == b"!" and m.base.keep_samples_path is None
    C.memset(C.byref(m), 0xFF, C.sizeof(m))
    bv.lib.bvcf_config_defaults(C.byref(m.base))
    assert m.base.reserved[0] == 0  # a plain config: nothing behind it is read
    assert bv.ConfigMore.pair_stats_path.offset == C.sizeof(bv.Config)
    c = bv.make_config({"relatedness": "/x/y"})
    assert c.reserved[0] == bv.CONFIG_MORE
    assert C.cast(C.byref(c), C.POINTER(bv.ConfigMore)).contents.pair_stats_path == b"/x/y"
    assert bv.make_config({}).reserved[0] == 0


def test_config_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\n'
                   "int main(){printf(\"%zu %zu %zu %zu\\n\", sizeof(bvcf_config), sizeof(bvcf_config_more),"
                   "offsetof(bvcf_config_more, pair_stats_path), offsetof(bvcf_config, reserved)); return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [C.sizeof(bv.Config), C.sizeof(bv.ConfigMore), bv.ConfigMore.pair_stats_path.offset, bv.Config.reserved.offset]


def test_abi_versions_stand(bv):
    assert bv.ABI_VERSION == 9 and bv.ABI_VERSION_SUBSET == 10
    with open(os.path.join(ROOT, "include", "bvcf.h")) as f:
        h = f.read()
    assert "#define BVCF_ABI_VERSION 9\n" in h and "#define BVCF_ABI_VERSION_SUBSET 10\n" in h


def test_cli_flag_without_a_value():
    p = subprocess.run([EXE, "--relatedness"], input=b"", capture_output=True, timeout=60)
    assert p.returncode == 2 and b"flag needs an argument: -relatedness" in p.stderr
