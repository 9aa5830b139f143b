"""--keepVariants / --excludeVariants, the parts that need no GPU: the list file's rules, the exported hash against FNV-1a
written out in Python, the invariants of the built table, bvcf_variant_gate_count on hand-made records, the ABI's layout,
the CLI's argument errors, and -- with the oracle alone -- that the inputs of tests/test_gpu_variant_list.py reach what
those tests are about."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import ldpairs
import oracle_lib as orc
import pairtable as pt
import sitegate as sg
import variantlist as vl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


# ---- the list file

def test_list_file_rules(bv):
    text = b"chr1:100:A:T\r\n\n\r\nchr1:100:A:T\n a b \nchr2:5:C:+ACG\r\r\n\tx\nlast"
    want = [b"chr1:100:A:T", b"chr1:100:A:T", b" a b ", b"chr2:5:C:+ACG\r", b"\tx", b"last"]
    assert vl.parse_list(text) == want
    t = bv.VariantTable(text=text)
    assert t.n == 5  # (the duplicate is stored once)
    for s in want:
        assert t.has(s), s
    for s in (b"a b", b" a b", b"a b ", b"chr2:5:C:+ACG", b"x", b"last\n", b"", b"chr1:100:A:T\r", b"chr1:100:A"):
        assert not t.has(s), s
    assert sorted(t.blob[e["off"]:e["off"] + e["len"]] for e in t.entries if e["len"]) == sorted(set(want))
    assert bv.VariantTable(text=b"x\n").n == bv.VariantTable(text=b"x").n == 1
    assert bv.VariantTable(text=b"\n\r\n\n").n == 0 and bv.VariantTable(text=b"").n == 0


def test_build_refuses_an_empty_entry(bv):
    with pytest.raises(bv.BvcfError) as ei:
        bv.VariantTable([b"a", b""])
    assert ei.value.rc == bv.E_ARG


# ---- the hash and the capacity rule

def test_locus_hash_is_fnv1a_64(bv):
    assert vl.fnv1a64(b"") == 0xcbf29ce484222325 and vl.fnv1a64(b"a") == 0xaf63dc4c8601ec8c  # the published vectors
    assert vl.fnv1a64(b"foobar") == 0x85944171f73967e8
    loci = vl.loci_of(orc.run(vl.kinds_vcf(5))[1])
    for s in [b"", b"a", b"foobar", bytes(range(256)), b"\xff" * 1000] + loci + vl.near_misses(loci):
        assert bv.locus_hash(s) == vl.fnv1a64(s), s


def test_capacity_rule(bv):
    for n in list(range(0, 70)) + [127, 128, 129, 10 ** 4, 10 ** 6, (1 << 26) - 1, 1 << 26, (1 << 26) + 1, 1 << 27]:
        cap = bv.variant_table_capacity(n)
        assert cap == vl.capacity_rule(n), n
        assert cap >= 16 and cap & (cap - 1) == 0 and cap >= 2 * n and (cap == 16 or cap < 4 * n)
    assert bv.variant_table_capacity((1 << 27) + 1) == 0 and bv.VARIANT_MAX_ENTRIES == 1 << 27


# ---- the built table

def check_table(bv, t, loci):
    """every invariant of a table built from loci"""
    distinct = sorted(set(loci))
    e = t.entries
    used = e[e["len"] > 0]
    cap = t.capacity
    assert t.n == len(distinct) == len(used) and cap == bv.variant_table_capacity(len(distinct)) == len(e)
    assert not e["zero"].any() and not e[e["len"] == 0]["tag"].any()
    blob = t.blob
    assert len(blob) == sum(len(x) for x in distinct)
    assert sorted(blob[x["off"]:x["off"] + x["len"]] for x in used) == distinct
    for slot in np.nonzero(e["len"])[0]:
        x = e[slot]
        s = blob[x["off"]:x["off"] + x["len"]]
        h = vl.fnv1a64(s)
        assert x["tag"] == h >> 32
        home = h & (cap - 1)
        k = home  # every slot from the home slot to the entry is taken: a probe from the home slot reaches it
        while k != slot:
            assert e[k]["len"] != 0
            k = (k + 1) & (cap - 1)
    for s in distinct:
        assert t.has(s), s
    for s in vl.near_misses(distinct) if all(x.count(b":") == 3 for x in distinct) else []:
        assert not t.has(s), s


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 16, 17, 1000, 20000])
def test_table_invariants(bv, n):
    loci = vl.rows_loci(n)
    check_table(bv, bv.VariantTable(loci + loci[: n // 2]), loci)
    assert not bv.VariantTable(loci).has(b"chr1:999:A:C")


def test_table_of_every_row_kind(bv):
    loci = vl.loci_of(orc.run(vl.kinds_vcf(5))[1])
    check_table(bv, bv.VariantTable(loci), loci)


def test_empty_table(bv):
    t = bv.VariantTable([])
    assert t.n == 0 and t.capacity == 16 and not t.entries["len"].any() and t.blob == b""
    assert not t.has(b"chr1:100:A:T") and not t.has(b"")


def test_probe_chain_wraps_around_the_end(bv):
    listed, every = vl.wrap_case(bv)
    loci = [vl.snp_locus(p) for p in listed]
    assert len(loci) == 4 and all(vl.fnv1a64(s) & 15 == 15 for s in loci)
    t = bv.VariantTable(loci)
    e = t.entries
    assert t.capacity == 16 and list(np.nonzero(e["len"])[0]) == [0, 1, 2, 15]
    at = [bytes(t.blob[e[k]["off"]:e[k]["off"] + e[k]["len"]]) for k in (15, 0, 1, 2)]
    assert at == loci  # in the order they were inserted: the chain 15, 0, 1, 2
    check_table(bv, t, loci)
    others = [vl.snp_locus(p) for p in every if p not in listed]
    assert {vl.fnv1a64(s) & 15 for s in others} == {15, 0, 3} and not any(t.has(s) for s in others)


def test_collision_pair_shares_tag_and_home_slot(bv):
    listed, in_file = vl.collision_case(bv)
    a, b = vl.collision_pair(bv)
    A, B = vl.snp_locus(a), vl.snp_locus(b)
    assert A != B and listed[0] == a and b in in_file and a not in in_file
    cap = bv.variant_table_capacity(len(listed))  # the capacity the list of the GPU test gets
    assert cap == 16
    ha, hb = bv.locus_hash(A), bv.locus_hash(B)
    assert ha != hb and ha >> 32 == hb >> 32 and ha & (cap - 1) == hb & (cap - 1)
    assert (ha, hb) == (vl.fnv1a64(A), vl.fnv1a64(B))
    t = bv.VariantTable([vl.snp_locus(p) for p in listed])
    assert t.capacity == cap and t.has(A) and not t.has(B)  # the same tag in the same home slot, and still not found
    home = ha & (cap - 1)
    assert t.entries[home]["tag"] == hb >> 32 and t.entries[home]["len"] == len(B)  # B's probe meets A's entry: tag and length agree
    # under the list, the file of the GPU test both keeps and drops
    mask = vl.select(orc.run(vl.snps_vcf(in_file))[1], [vl.snp_locus(p) for p in listed], False)
    assert mask == [p in listed for p in in_file] and any(mask) and not all(mask)


# ---- bvcf_variant_gate_count

def test_variant_gate_count_on_hand_made_records(bv):
    lines = np.zeros(5, dtype=bv.LINE_DTYPE)
    alleles = np.zeros(8, dtype=bv.ALLELE_DTYPE)
    # line 0: one row, kept.  line 1: three rows -- dropped by the list, kept and then failed by the site gate, kept
    # line 2: FILTER verdict, its record slot holds leftovers.  line 3: a row no sample carries.  line 4: dropped
    lines["status"] = [bv.LINE_OK, bv.LINE_OK, bv.LINE_FILTER, bv.LINE_OK, bv.LINE_OK]
    lines["n_rec"] = [1, 3, 0, 1, 1]
    lines["rec_first"] = [0, 5, 0, 0, 0]
    alleles["ac"] = [3, 0, 7, 0, 0, 0, 2, 9]
    alleles["pad"][:, 1] = [0, 1, 1, 0, 1, 0, 0, 1]
    alleles["pad"][:, 0] = [0, 0, 0, 0, 0, bv.GATE_MIN_MAC, 0, 0]
    r = bv.Result()
    r.status, r.n_lines, r.n_alleles, r.n_samples = 0, 5, 8, 4
    r.lines, r.alleles = lines.ctypes.data, alleles.ctypes.data
    assert bv.variant_gate_count(r) == [5, 3, 2]
    assert bv.site_gate_count(r)[:2] == [3, 2]  # the rows the list took out are not the gate's
    r.n_samples = 0
    assert bv.variant_gate_count(r) == [0, 0, 0]
    r.n_samples, r.status = 4, bv.E_CAPACITY
    assert bv.variant_gate_count(r) == [0, 0, 0]


# ---- the ABI

def test_header_binding_and_library_agree(bv):
    with open(os.path.join(ROOT, "include", "bvcf.h")) as f:
        h = f.read()
    for decl in (r"uint64_t bvcf_locus_hash\(const char \*s, size_t n\);", r"uint64_t bvcf_variant_table_capacity\(uint64_t n\);",
                 r"int bvcf_set_variant_list\(bvcf_ctx \*ctx, const char \*bytes, const uint64_t \*off, const uint32_t \*len, uint64_t n, int exclude\);",
                 r"void bvcf_variant_gate_count\(const bvcf_result \*r, uint64_t out\[3\]\);",
                 r"void bvcf_config_variants_defaults\(bvcf_config_variants \*c\);"):
        assert re.search(decl, h), decl
    assert "#define BVCF_CONFIG_MORE_VARIANTS 5\n" in h and bv.CONFIG_MORE_VARIANTS == 5
    for name in ("bvcf_locus_hash", "bvcf_variant_table_capacity", "bvcf_variant_table_build", "bvcf_variant_table_parse",
                 "bvcf_variant_table_free", "bvcf_variant_table_has", "bvcf_set_variant_table", "bvcf_set_variant_list",
                 "bvcf_variant_gate_count", "bvcf_config_variants_defaults"):
        assert name in bv.EXPORTS and hasattr(bv.lib, name)
    for name in ("bvcf_bench_variant_kernel", "bvcf_bench_variant_gate_stride"):
        assert name in bv.BENCH_EXPORTS and hasattr(bv.lib, name)
    assert bv.VARIANT_REPORT == vl.REPORT
    assert bv.ABI_VERSION == 9 and bv.ABI_VERSION_SUBSET == 10


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    fields = ["keep_variants_path", "exclude_variants_path", "variant_filter_path"]
    tf = ["entries", "capacity", "blob", "blob_bytes", "n"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu", sizeof(bvcf_config_ld), sizeof(bvcf_config_variants), sizeof(bvcf_variant_table),'
                   "sizeof(bvcf_allele), offsetof(bvcf_allele, pad));"
                   + "".join('printf(" %%zu", offsetof(bvcf_config_variants, %s));' % f for f in fields)
                   + "".join('printf(" %%zu", offsetof(bvcf_variant_table, %s));' % f for f in tf)
                   + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    V, T = bv.ConfigVariants, bv.VariantTableStruct
    assert out == [C.sizeof(bv.ConfigLd), C.sizeof(V), C.sizeof(T), 64, 54] + [getattr(V, f).offset for f in fields] + \
        [getattr(T, f).offset for f in tf]
    assert V.keep_variants_path.offset == C.sizeof(bv.ConfigLd) and V.ld.offset == 0
    assert bv.ALLELE_DTYPE.fields["pad"][1] == 54 and bv.VARIANT_ENTRY_DTYPE.itemsize == 16


def test_older_defaults_write_what_they_wrote(bv):
    """each older *_defaults leaves everything behind its own struct alone; the new one fills the whole struct"""
    V = bv.ConfigVariants
    older = ((bv.lib.bvcf_config_more_defaults, bv.ConfigMore.site_gate.offset, 0),
             (bv.lib.bvcf_config_gate_defaults, bv.ConfigMore.plink_prefix.offset, bv.CONFIG_MORE_GATE),
             (bv.lib.bvcf_config_plink_defaults, C.sizeof(bv.ConfigMore), bv.CONFIG_MORE_PLINK),
             (bv.lib.bvcf_config_trios_defaults, C.sizeof(bv.ConfigTrios), bv.CONFIG_MORE_TRIOS),
             (bv.lib.bvcf_config_ld_defaults, C.sizeof(bv.ConfigLd), bv.CONFIG_MORE_LD))
    for fn, first_untouched, marker in older:
        v = V()
        C.memset(C.byref(v), 0xFF, C.sizeof(v))
        fn(C.byref(v))
        assert bytes(v)[first_untouched:] == b"\xff" * (C.sizeof(v) - first_untouched), fn
        assert v.ld.trios.more.base.reserved[0] == bv.CONFIG_MORE and v.ld.trios.more.base.reserved[1] == marker
    ld = bv.ConfigLd()
    bv.lib.bvcf_config_ld_defaults(C.byref(ld))
    v = V()
    C.memset(C.byref(v), 0xFF, C.sizeof(v))
    bv.lib.bvcf_config_variants_defaults(C.byref(v))
    assert v.ld.trios.more.base.reserved[1] == bv.CONFIG_MORE_VARIANTS
    assert v.keep_variants_path is None and v.exclude_variants_path is None and v.variant_filter_path is None
    assert (v.ld.ld_window, v.ld.ld_t6, v.ld.ld_t6_set, v.ld.ld_path, v.ld.ld_prune_prefix) == (50, 200000, 1, None, None)
    # but for the marker, its head is what bvcf_config_ld_defaults makes
    v.ld.trios.more.base.reserved[1] = bv.CONFIG_MORE_LD
    assert bytes(v)[:C.sizeof(ld)] == bytes(ld)


def test_config_markers(bv):
    assert list(bv.make_config({}).reserved) == [0, 0]
    assert list(bv.make_config({"ldPrune": "/x"}).reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_LD]
    for key, field in (("keepVariants", "keep_variants_path"), ("excludeVariants", "exclude_variants_path"),
                       ("variantFilterReport", "variant_filter_path")):
        c = bv.make_config({key: "/x/y", "minMac": 3})
        assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_VARIANTS]
        v = C.cast(C.byref(c), C.POINTER(bv.ConfigVariants)).contents
        assert getattr(v, field) == b"/x/y" and v.ld.trios.more.site_gate.min_mac == 3 and v.ld.ld_window == 50
        assert [v.keep_variants_path, v.exclude_variants_path, v.variant_filter_path].count(None) == 2


# ---- the CLI's argument errors (no device is reached)

def cli(args, stdin_bytes=b""):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=60)


def test_cli_both_flags(tmp_path):
    p = cli(["--keepVariants", str(tmp_path / "a"), "--excludeVariants", str(tmp_path / "b")])
    assert p.returncode == 2 and p.stdout == b""
    assert p.stderr == b"-keepVariants and -excludeVariants cannot both be given\n"


@pytest.mark.parametrize("flag", ["keepVariants", "excludeVariants", "variantFilterReport"])
def test_cli_flag_without_a_value(flag):
    p = cli(["--" + flag])
    assert p.returncode == 2 and p.stdout == b""
    assert p.stderr == ("flag needs an argument: -%s\n" % flag).encode()


@pytest.mark.parametrize("flag", ["keepVariants", "excludeVariants"])
def test_cli_empty_path(flag):
    p = cli(["--%s=" % flag])
    assert p.returncode == 2 and p.stderr.count(b"\n") == 1 and ('invalid value "" for flag -%s: want' % flag).encode() in p.stderr


@pytest.mark.parametrize("flag", ["keepVariants", "excludeVariants"])
def test_cli_unreadable_list(flag, tmp_path):
    """one message and exit code 1, before the input is looked at or a device asked for"""
    bad = tmp_path / "no_such_dir" / "list.txt"
    p = cli(["--" + flag, str(bad)], vl.rows_vcf(5))
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.count(b"\n") == 1 and str(bad).encode() in p.stderr and b"No such file" in p.stderr


def test_cli_unwritable_report(tmp_path):
    bad = tmp_path / "no_such_dir" / "x.report"
    p = cli(["--variantFilterReport", str(bad)], vl.rows_vcf(5))
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.count(b"\n") == 1 and str(bad).encode() in p.stderr


# ---- the conditions on the inputs of tests/test_gpu_variant_list.py, with the oracle alone

def oracle_body(vcf, cfg=None):
    rc, body, _, _ = orc.run(vcf, cfg or {})
    assert rc == 0
    return body


def keeps_and_drops(body, loci):
    for exclude in (False, True):
        mask = vl.select(body, loci, exclude)
        assert any(mask) and not all(mask), "a list that does not both keep and drop"


@pytest.mark.parametrize("ns", [1, 5])
def test_kinds_input_has_every_kind(ns):
    body = oracle_body(vl.kinds_vcf(ns))
    loci = vl.loci_of(body)
    rows = [r.split(b"\t") for r in vl.rows_of(body)]
    types = {r[pt.BASE_HEADER.index("type")] for r in rows}
    assert {b"SNP", b"INS", b"DEL", b"MNP", b"MULTIALLELIC"} <= types
    alts = [x.split(b":")[3] for x in loci]
    assert set(vl.INS_LENGTHS) <= {len(a) - 1 for a in alts if a.startswith(b"+")}
    assert {b"-%d" % n for n in vl.DEL_LENGTHS} <= set(alts)
    assert {x.split(b":")[0] for x in loci} >= {b"chr1", b"chrc", b"chrcat", b"chrom", b"chrX", b"chrUn_gl000220"}
    assert loci.count(b"chr1:100:A:T") == 2 and b"chr1:1000:A:T" in loci  # `1` and `chr1`: one locus, two rows
    assert b"chr1:00100:A:T" in loci                                      # the POS bytes as they stand
    assert b"chr3:2000:A:+AC" in loci and b"chr3:2000:A:+ACG" in loci and b"chr4:9001:C:-9" in loci and b"chr4:9001:C:-8" in loci
    assert {b"chr2:200:A:C", b"chr2:200:A:G"} <= set(loci) and (b"chr2:200:A:T" in loci) == (ns == 5)
    assert not any(x.startswith(b"chr5:100:") for x in loci)              # the line no sample carries gives no row
    assert any(len(x.split(b":")[1]) == 10 for x in loci)
    misses = vl.near_misses(sorted(set(loci)))
    assert len(misses) > 5 * len(set(loci)) and not set(misses) & set(loci)
    assert b"1:100:A:T" in misses and b"chr1:100:A:TT" in misses and b"chr3:2000:A:+A" in misses and b"chr1:10:A:T" in misses
    lists = vl.kinds_lists(loci)
    assert sorted(lists[0] + lists[1]) == sorted(set(loci)) and not set(lists[0]) & set(lists[1])
    for lst in lists:
        keeps_and_drops(body, lst + misses)
    for x, y in vl.KIND_PAIRS:  # loci that differ by a suffix, or are the ALTs of one line, fall on different sides
        assert x in lists[0] and y in lists[1]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_run_shape_inputs(n):
    body = oracle_body(vl.rows_vcf(n))
    assert vl.loci_of(body) == vl.rows_loci(n)  # one row per line, every row carried
    if n > 1:
        keeps_and_drops(body, vl.third_of(n))
    else:
        assert vl.select(body, vl.third_of(1), False) == [True] and vl.select(body, vl.third_of(1), True) == [False]


def test_wrap_input_keeps_and_drops(bv):
    listed, every = vl.wrap_case(bv)
    keeps_and_drops(oracle_body(vl.snps_vcf(every)), [vl.snp_locus(p) for p in listed])


def test_composition_inputs_keep_and_drop():
    for vcf in (sg.case_input("sweep"), sg.case_input("fuzz13"), sg.case_input("masked13"), sg.case_input("rare300"),
                sg.case_input("cut300"), vl.pedigree_case()[0], vl.round_trip_input()[0]):
        body = oracle_body(vcf)
        keeps_and_drops(body, vl.every_other(vl.loci_of(body)))


def test_round_trip_input_has_no_duplicate_locus():
    vcf, window = vl.round_trip_input()
    body = oracle_body(vcf)
    loci = vl.loci_of(body)
    assert len(loci) == len(set(loci)) > 100
    want = ldpairs.expected_from_body(body, pt.sample_names(vcf), window, 200000, with_table=False)
    assert 0 < int(want["kept"].sum()) < len(loci)  # the prune both keeps and drops


def test_golden_list_keeps_and_drops():
    vcf = gzip.decompress(open(GOLDEN_GZ, "rb").read())
    body = oracle_body(vcf)
    lst = vl.golden_list(body)
    assert 9000 < len(lst) < 11000
    keeps_and_drops(body, lst)
