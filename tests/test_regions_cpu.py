"""--regions / --excludeRegions, the parts that need no GPU: the SPEC and BED rules with every error case, merging, the
device's lookup run on the host (bvcf_region_table_has) against the naive reference of tests/regions.py, the pos text rule,
bvcf_region_gate_count and the changed bvcf_variant_gate_count on hand-made records, the ABI's layout, the CLI's argument
errors, and -- with the oracle alone -- that the inputs of tests/test_gpu_regions.py both keep and drop rows of each kind."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
import regions as rg
import sitegate as sg
import variantlist as vl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


# ---- SPECs

SPECS = [(b"chr1", (b"chr1", 1, rg.MAX_COORD)), (b"1", (b"chr1", 1, rg.MAX_COORD)), (b"1:100", (b"chr1", 100, 100)),
         (b"chr1:100-200", (b"chr1", 100, 200)), (b"1:100-", (b"chr1", 100, rg.MAX_COORD)), (b"X:5-5", (b"chrX", 5, 5)),
         (b"c", (b"chrc", 1, rg.MAX_COORD)), (b"cat:7", (b"chrcat", 7, 7)), (b"chrom:7", (b"chrom", 7, 7)),
         (b"1:007-0010", (b"chr1", 7, 10)), (b"1:" + b"9" * 18, (b"chr1", 10 ** 18 - 1, 10 ** 18 - 1)),
         # a tail that is not D, D- or D-D: the whole SPEC is a chromosome name
         (b"HLA:DRB1", (b"chrHLA:DRB1", 1, rg.MAX_COORD)), (b"ctg:5:100-200", (b"ctg:5", 100, 200)), (b"ctg:5", (b"chrctg", 5, 5)),
         (b"1:0", (b"chr1:0", 1, rg.MAX_COORD)), (b"1:0-5", (b"chr1:0-5", 1, rg.MAX_COORD)), (b"1:5-0", (b"chr1:5-0", 1, rg.MAX_COORD)),
         (b"1:-5", (b"chr1:-5", 1, rg.MAX_COORD)), (b"1:+5", (b"chr1:+5", 1, rg.MAX_COORD)), (b"1:1e5", (b"chr1:1e5", 1, rg.MAX_COORD)),
         (b"1: 5", (b"chr1: 5", 1, rg.MAX_COORD)), (b"1:5 ", (b"chr1:5 ", 1, rg.MAX_COORD)), (b"1:1,000", None),
         (b"1:" + b"9" * 19, (b"chr1:" + b"9" * 19, 1, rg.MAX_COORD)), (b"1:5-6-7", (b"chr1:5-6-7", 1, rg.MAX_COORD)),
         (b"1:", (b"chr1:", 1, rg.MAX_COORD)), (b"chr1:5--", (b"chr1:5--", 1, rg.MAX_COORD)), (b"cccc:", (b"cccc:", 1, rg.MAX_COORD))]


def table_sets(t):
    return t.merged(False), t.merged(True)


@pytest.mark.parametrize("spec,want", [x for x in SPECS if x[1] is not None])
def test_spec_forms(bv, spec, want):
    assert rg.parse_spec(spec) == want
    for exclude in (False, True):
        t = bv.RegionTable(**{"exclude" if exclude else "keep": spec})
        assert table_sets(t)[exclude] == {want[0]: [(want[1], want[2])]} and table_sets(t)[not exclude] == {}
        assert t.keep_given == (not exclude) and (t.n_keep, t.n_exclude) == ((0, 1) if exclude else (1, 0)) and t.n_chroms == 1


def test_spec_lists(bv):
    text = b"1:100-200,chr2,HLA:DRB1,1:150-300,ctg:5:7"
    want = rg.parse_specs(text)
    assert want == [(b"chr1", 100, 200), (b"chr2", 1, rg.MAX_COORD), (b"chrHLA:DRB1", 1, rg.MAX_COORD), (b"chr1", 150, 300), (b"ctg:5", 7, 7)]
    assert bv.RegionTable(keep=text).merged() == rg.merged(want)
    # (a separator inside a number splits the SPEC: "1:1,000" is chr1:1 and the chromosome "000")
    assert rg.parse_specs(b"1:1,000") == [(b"chr1", 1, 1), (b"chr000", 1, rg.MAX_COORD)]
    assert bv.RegionTable(keep=b"1:1,000").merged() == {b"chr1": [(1, 1)], b"chr000": [(1, rg.MAX_COORD)]}


@pytest.mark.parametrize("text", [b"", b",", b"chr1,", b",chr1", b"chr1,,chr2", b":100", b":100-200", b"chr1,:5-", b"1:200-100", b"chr1:5-4",
                                  b"chr2,1:" + b"9" * 18 + b"-1"])
def test_spec_errors(bv, text):
    with pytest.raises(rg.SpecError):
        rg.parse_specs(text)
    for exclude in (False, True):
        with pytest.raises(bv.BvcfError) as ei:
            bv.RegionTable(**{"exclude" if exclude else "keep": text})
        assert ei.value.rc == bv.E_ARG and len(str(ei.value)) > len("bvcf error -1: ")


def test_a_failed_parse_leaves_the_table_as_it_was(bv):
    t = bv.RegionTable(keep=b"chr1:5-9")
    err = C.create_string_buffer(64)
    assert bv.lib.bvcf_region_table_parse_specs(C.byref(t.t), b"chr2,chr3:9-1", 13, 0, err, 64) == bv.E_ARG and err.value
    assert bv.lib.bvcf_region_table_parse_bed(C.byref(t.t), b"chr4\t1\t2\nchr5\t1\n", 16, 1, err, 64) == bv.E_ARG and b"line 2" in err.value
    assert bv.lib.bvcf_region_table_build(C.byref(t.t)) == 0
    assert table_sets(t) == ({b"chr1": [(5, 9)]}, {}) and t.n_chroms == 1
    # a short message buffer is filled and terminated
    small = C.create_string_buffer(b"\xff" * 8, 8)
    assert bv.lib.bvcf_region_table_parse_specs(C.byref(t.t), b"1:9-1", 5, 0, small, 8) == bv.E_ARG and small.raw[7:] == b"\0"


# ---- BED

BED = (b"# a comment\ntrack name=x\nbrowser position chr1\n\n\r\n"
       b"chr1\t99\t200\n1\t149\t300\tname\t0\t+\r\nchr2\t0\t1\nchr2\t5\t5\nX\t0\t" + b"9" * 18 + b"\nHLA:DRB1\t10\t20\nchr1\t0099\t0100\n"
       b"chr3\t7\t8")


def test_bed_rules(bv):
    want = rg.parse_bed(BED)
    assert want == [(b"chr1", 100, 200), (b"chr1", 150, 300), (b"chr2", 1, 1), (b"chrX", 1, 10 ** 18 - 1), (b"chrHLA:DRB1", 11, 20),
                    (b"chr1", 100, 100), (b"chr3", 8, 8)]
    t = bv.RegionTable(keep_bed=BED)
    assert t.merged() == rg.merged(want) == {b"chr1": [(100, 300)], b"chr2": [(1, 1)], b"chrX": [(1, 10 ** 18 - 1)],
                                            b"chrHLA:DRB1": [(11, 20)], b"chr3": [(8, 8)]}
    assert t.n_keep == 5 and t.n_exclude == 0 and t.keep_given
    # an empty file, and a file of ignored lines, is a keep set that is empty
    for text in (b"", b"\n\n", b"#x\ntrack\nbrowser\nchr1\t5\t5\n"):
        t = bv.RegionTable(keep_bed=text)
        assert t.keep_given and t.n_keep == 0 and t.n_chroms == 0 and t.capacity == 16
        assert not t.stays(b"chr1", b"5", b"T")
        t = bv.RegionTable(exclude_bed=text)
        assert not t.keep_given and t.n_exclude == 0 and t.stays(b"chr1", b"5", b"T")


@pytest.mark.parametrize("text,line", [(b"chr1\t1\n", 1), (b"chr1\n", 1), (b"chr1 1 2\n", 1), (b"chr1\t1\t2\nchr1\t1", 2), (b"#c\n\nchr1\t\t5\n", 3),
                                       (b"chr1\t1\t\n", 1), (b"chr1\t-1\t5\n", 1), (b"chr1\t1\t+5\n", 1), (b"chr1\t1e2\t500\n", 1),
                                       (b"chr1\t1\t5 \n", 1), (b"chr1\t1\t" + b"9" * 19 + b"\n", 1), (b"chr1\t" + b"0" * 19 + b"\t5\n", 1),
                                       (b"chr1\t1\t2\r\nchr1\t6\t5\r\n", 2), (b"chr1\t1\t2\n" * 9 + b"x\ty\tz\n", 10)])
def test_bed_errors_name_the_line(bv, text, line):
    with pytest.raises(rg.BedError) as ri:
        rg.parse_bed(text)
    assert ri.value.line_no == line
    for key in ("keep_bed", "exclude_bed"):
        with pytest.raises(bv.BvcfError) as ei:
            bv.RegionTable(**{key: text})
        assert ei.value.rc == bv.E_ARG and ("line %d:" % line) in str(ei.value)


def test_more_than_the_bound_of_names(bv):
    n = bv.REGION_MAX_CHROMS
    text = b"".join(b"k%d\t0\t1\n" % i for i in range(n))
    t = bv.RegionTable(exclude_bed=text)
    assert t.n_chroms == n and t.capacity == 2 * n and t.has(b"k%d" % (n - 1), b"1", b"T") == 2 and t.has(b"k%d" % n, b"1", b"T") == 0
    with pytest.raises(bv.BvcfError) as ei:
        bv.RegionTable(exclude_bed=text + b"one_more\t0\t1\n")
    assert ei.value.rc == bv.E_TOO_BIG and "1048576" in str(ei.value)


# ---- merging

def test_merging(bv):
    iv = [(b"chr1", 10, 20), (b"chr1", 15, 30),   # overlapping
          (b"chr1", 31, 40),                        # abutting
          (b"chr1", 42, 50),                        # one base apart: stays apart
          (b"chr1", 44, 46),                        # nested
          (b"chr1", 42, 50), (b"chr1", 42, 50),     # duplicates
          (b"chr1", 60, 60), (b"chr1", 61, 61), (b"chr1", 59, 59), (b"chr1", 1, 1), (b"chr1", 3, 3),
          (b"chr2", 5, 9), (b"chr2", 1, 4), (b"chr3", 7, 7)]
    want = {b"chr1": [(1, 1), (3, 3), (10, 40), (42, 50), (59, 61)], b"chr2": [(1, 9)], b"chr3": [(7, 7)]}
    assert rg.merged(iv) == rg.painted(iv, 100) == want
    rng = random.Random(31)
    for _ in range(5):
        rng.shuffle(iv)
        t = bv.RegionTable(keep_bed=rg.bed_text(iv[:8]), keep=b",".join(b"%s:%d-%d" % x for x in iv[8:]), exclude_bed=rg.bed_text(iv))
        assert table_sets(t) == (want, want) and t.n_keep == t.n_exclude == 7 and t.n_chroms == 3
    # open ends swallow what follows; a whole chromosome swallows everything
    t = bv.RegionTable(keep=b"1:100-,1:50-60,1:99,1:5000-6000,2:7,2")
    assert t.merged() == {b"chr1": [(50, 60), (99, rg.MAX_COORD)], b"chr2": [(1, rg.MAX_COORD)]}
    # the two sets do not merge into each other
    t = bv.RegionTable(keep=b"1:10-20", exclude=b"1:15-30,1:21")
    assert table_sets(t) == ({b"chr1": [(10, 20)]}, {b"chr1": [(15, 30)]})


@pytest.mark.parametrize("seed", range(6))
def test_seeded_merges_against_painting(bv, seed):
    rng = random.Random(700 + seed)
    iv = []
    for _ in range(rng.choice([1, 2, 3, 17, 64, 200])):
        b = rng.randint(1, 380)
        iv.append((rng.choice([b"chr1", b"chr2", b"chrom"]), b, b + rng.choice([0, 0, 1, 2, 5, 20])))
    t = bv.RegionTable(exclude_bed=rg.bed_text(iv))
    assert t.merged(True) == rg.painted(iv, 400) == rg.merged(iv)


def check_table(bv, t):
    """the invariants of a built table"""
    ch, iv, blob, cap = t.chroms, t.intervals, t.blob, t.capacity
    used = ch[ch["len"] > 0]
    assert cap == bv.variant_table_capacity(t.n_chroms) == len(ch) and len(used) == t.n_chroms and not ch["zero"].any()
    assert len(iv) == t.n_keep + t.n_exclude == int(used["n"].sum())
    seen = np.zeros(len(iv), dtype=int)
    for slot in np.nonzero(ch["len"])[0]:
        x = ch[slot]
        name = blob[x["off"]:x["off"] + x["len"]]
        h = vl.fnv1a64(name)
        assert x["tag"] == h >> 32 and rg.norm(name) == name
        k = h & (cap - 1)
        while k != slot:
            assert ch[k]["len"] != 0
            k = (k + 1) & (cap - 1)
        for s in (0, 1):
            mine = iv[int(x["first"][s]):int(x["first"][s]) + int(x["n"][s])]
            seen[int(x["first"][s]):int(x["first"][s]) + int(x["n"][s])] += 1
            assert (mine["beg"] <= mine["end"]).all() and (mine["end"][:-1] + 1 < mine["beg"][1:]).all()
    assert (seen == 1).all()


# ---- the lookup against the naive reference

POS_TEXTS = [b"007", b"0", b"1", b"9" * 18, b"9" * 19, b"0" * 18 + b"7", b"-5", b"-0", b"-", b"+5", b"1e5", b"", b" 5", b"5 ", b"5.0",
             b"-" + b"9" * 18, b"-" + b"9" * 19, b"0x10", b"12a", b"--5"]


def test_pos_text_rule(bv):
    assert [rg.pos_of(p) for p in POS_TEXTS] == [7, 0, 1, 10 ** 18 - 1, None, None, -5, 0, None, None, None, None, None, None, None,
                                                 -(10 ** 18 - 1), None, None, None, None]
    # every chromosome whole, from the smallest coordinate a region can name: a position >= 1 overlaps, nothing else does
    t = bv.RegionTable(keep=b"chr1", exclude=b"chr1:1-")
    for p in POS_TEXTS:
        want = 3 if (rg.pos_of(p) is not None and rg.pos_of(p) >= 1) else 0
        assert t.has(b"chr1", p, b"T") == t.has(b"1", p, b"T") == want, p
        assert t.has(b"chr1", p, b"-3") == (3 if (rg.pos_of(p) is not None and rg.pos_of(p) + 2 >= 1) else 0), p
    # a row without a position overlaps nothing: --regions drops it, --excludeRegions keeps it
    assert not bv.RegionTable(keep=b"chr1").stays(b"chr1", b"1e5", b"T") and bv.RegionTable(exclude=b"chr1").stays(b"chr1", b"1e5", b"T")
    # a deletion that starts at a negative position and reaches base 1
    t = bv.RegionTable(keep=b"chr1:1")
    assert [t.has(b"chr1", b"-5", a) for a in (b"-6", b"-7", b"-8", b"T", b"+ACGTACGT")] == [0, 1, 1, 0, 0]
    assert [t.has(b"chr1", b"0", a) for a in (b"-1", b"-2", b"T")] == [0, 1, 0]
    assert [t.has(b"chr1", b"1", a) for a in (b"-1", b"T", b"+A", b"-", b"-x", b"--1")] == [1, 1, 1, 1, 1, 1]


def test_spans_at_the_edges(bv):
    t = bv.RegionTable(keep=b"1:1000-2000,1:3000", exclude=b"1:" + b"9" * 18)
    cases = [(b"999", b"T", 0), (b"1000", b"T", 1), (b"2000", b"T", 1), (b"2001", b"T", 0), (b"3000", b"+ACG", 1), (b"2999", b"+ACG", 0),
             (b"995", b"-5", 0), (b"995", b"-6", 1), (b"2000", b"-1", 1), (b"2001", b"-999", 0), (b"2001", b"-1000", 1), (b"2995", b"-10", 1),
             (b"2995", b"-5", 0), (b"2995", b"-6", 1), (b"3001", b"-4294967295", 0), (b"9" * 18, b"T", 2), (b"9" * 17 + b"8", b"-2", 2),
             (b"9" * 17 + b"8", b"-1", 0), (b"1", b"-4294967295", 1), (b"1", b"-99999999999", 1)]
    for pos, alt, want in cases:
        assert t.has(b"1", pos, alt) == want == rg.has_bits(rg.parse_specs(b"1:1000-2000,1:3000"), rg.parse_specs(b"1:" + b"9" * 18), b"chr1", pos, alt), (pos, alt)


@pytest.mark.parametrize("seed", range(8))
def test_lookup_against_the_naive_reference(bv, seed):
    rng = random.Random(900 + seed)
    chroms = [b"1", b"chr1", b"chr10", b"M", b"chrM", b"c", b"chrom", b"HLA:DRB1", b"chrUn_gl000220_random", b"22", b"X"]
    n_iv = rng.choice([0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 500])

    def some(n):
        out = []
        for _ in range(n):
            b = rng.randint(1, 3000)
            out.append((rg.norm(rng.choice(chroms[:8])), b, b + rng.choice([0, 0, 1, 3, 10, 100])))
        return out

    keep, excl = some(n_iv), some(rng.choice([0, 1, 5, 40]))
    keep_given = bool(keep) or seed % 2 == 0
    t = bv.RegionTable(keep_bed=rg.bed_text(keep) if keep_given else None, exclude_bed=rg.bed_text(excl))
    check_table(bv, t)
    assert (t.merged(False), t.merged(True)) == (rg.merged(keep), rg.merged(excl))
    edges = sorted({x for _, b, e in keep + excl for x in (b - 1, b, e, e + 1)})
    probes = [(c, b"%d" % p, a) for c in chroms for p in rng.sample(edges, min(len(edges), 40)) + [rng.randint(-5, 3200) for _ in range(20)]
              for a in (b"T", b"+AC", b"-1", b"-2", b"-%d" % rng.randint(3, 150))]
    probes += [(c, p, b"-40") for c in chroms[:3] for p in POS_TEXTS]
    for c, p, a in probes:
        want = rg.has_bits(keep, excl, rg.norm(c), p, a)
        assert t.has(c, p, a) == want, (c, p, a)
        assert t.stays(c, p, a) == rg.stays(keep if keep_given else None, excl, rg.norm(c), p, a)


def test_names(bv):
    t = bv.RegionTable(keep=rg.NAMES_KEEP, exclude=rg.NAMES_EXCLUDE)
    check_table(bv, t)
    assert [t.has(c, b"200", b"T") for c in (b"1", b"chr1", b"10", b"chr10", b"chr100", b"chr", b"", b"M", b"chrM", b"m")] == [3, 3, 1, 1, 0, 0, 0, 1, 1, 0]
    assert [t.has(b"chr10", p, b"T") for p in (b"199", b"200", b"201")] == [0, 1, 0]
    assert t.has(b"HLA:DRB1", b"1", b"T") == 1 and t.has(b"chrHLA:DRB1", b"1", b"T") == 1 and t.has(b"HLA", b"1", b"T") == 0
    assert t.has(b"ctg:5", b"150", b"T") == 1 and t.has(b"ctg:5", b"5", b"T") == 0 and t.has(b"ctg", b"5", b"T") == 1 and t.has(b"chrctg", b"5", b"T") == 1
    assert t.has(b"X", b"1", b"T") == 2 and t.has(b"cat", b"299", b"T") == 1 and t.has(b"cat", b"299", b"-2") == 3 and t.has(b"2", b"200", b"T") == 0
    assert t.has(b"chrUn_gl000220_random", b"250", b"T") == 1 and t.has(b"chrUn_gl000220_randoM", b"250", b"T") == 0
    assert t.has(b"chrUn_gl000220_random_and_longer_than_every_name", b"250", b"T") == 0


def test_probe_chain_wraps_around_the_end(bv):
    listed, every = rg.wrap_case(bv)
    names = [rg.ctg(i) for i in listed]
    assert len(names) == 4 and all(vl.fnv1a64(s) & 15 == 15 for s in names)
    t = bv.RegionTable(keep=b",".join(names))
    ch = t.chroms
    assert t.capacity == 16 and list(np.nonzero(ch["len"])[0]) == [0, 1, 2, 15]
    check_table(bv, t)
    others = [rg.ctg(i) for i in every if i not in listed]
    assert {vl.fnv1a64(s) & 15 for s in others} == {15, 0, 3}
    assert all(t.has(s, b"100", b"T") == 1 for s in names) and not any(t.has(s, b"100", b"T") for s in others)


def test_collision_pair_shares_tag_and_home_slot(bv):
    listed, in_file = rg.collision_case(bv)
    a, b = rg.collision_pair(bv)
    A, B = rg.ctg(a), rg.ctg(b)
    assert A != B and listed[0] == a and b in in_file and a not in in_file and len(A) == len(B)
    ha, hb = bv.locus_hash(A), bv.locus_hash(B)
    assert ha != hb and ha >> 32 == hb >> 32 and ha & 15 == hb & 15 and (ha, hb) == (vl.fnv1a64(A), vl.fnv1a64(B))
    t = bv.RegionTable(keep=b",".join(rg.ctg(i) for i in listed))
    assert t.capacity == 16 and t.has(A, b"100", b"T") == 1 and t.has(B, b"100", b"T") == 0  # the same tag in the same home slot: not found
    home = ha & 15
    assert t.chroms[home]["tag"] == hb >> 32 and t.chroms[home]["len"] == len(B)
    mask = rg.select(oracle_body(rg.ctg_vcf(in_file)), rg.Sets(regions=b",".join(rg.ctg(i) for i in listed)))
    assert mask == [i in listed for i in in_file] and any(mask) and not all(mask)


# ---- the counts

def test_gate_counts_on_hand_made_records(bv):
    lines = np.zeros(5, dtype=bv.LINE_DTYPE)
    alleles = np.zeros(9, dtype=bv.ALLELE_DTYPE)
    # line 0: one row, kept by all.  line 1: four rows -- dropped by the regions, dropped by the list, kept and then failed by
    # the site gate, kept.  line 2: FILTER verdict, its record slot holds leftovers.  line 3: a row no sample carries.
    # line 4: dropped by the regions
    lines["status"] = [bv.LINE_OK, bv.LINE_OK, bv.LINE_FILTER, bv.LINE_OK, bv.LINE_OK]
    lines["n_rec"] = [1, 4, 0, 1, 1]
    lines["rec_first"] = [0, 5, 0, 0, 0]
    alleles["ac"] = [3, 0, 7, 0, 0, 0, 0, 2, 9]
    alleles["pad"][:, 1] = [0, 2, 2, 0, 2, 1, 0, 0, 2]
    alleles["pad"][:, 0] = [0, 0, 0, 0, 0, 0, bv.GATE_MIN_MAC, 0, 0]
    r = bv.Result()
    r.status, r.n_lines, r.n_alleles, r.n_samples = 0, 5, 9, 4
    r.lines, r.alleles = lines.ctypes.data, alleles.ctypes.data
    assert bv.region_gate_count(r) == [6, 4, 2]
    assert bv.variant_gate_count(r) == [4, 3, 1]  # the rows the regions took out are not the list's: bit 0 alone counts as dropped
    assert bv.site_gate_count(r)[:2] == [3, 2]    # ... nor the gate's
    r.n_samples = 0
    assert bv.region_gate_count(r) == [0, 0, 0]
    r.n_samples, r.status = 4, bv.E_CAPACITY
    assert bv.region_gate_count(r) == [0, 0, 0]
    # without regions pad[1] is 0 or 1 and the list's counts are what they were
    alleles["pad"][:, 1] = [0, 1, 1, 0, 1, 1, 0, 0, 1]
    r.status = 0
    assert bv.variant_gate_count(r) == [6, 3, 3] and bv.region_gate_count(r) == [6, 6, 0]


# ---- the ABI

def test_header_binding_and_library_agree(bv):
    with open(os.path.join(ROOT, "include", "bvcf.h")) as f:
        h = f.read()
    for decl in (r"int bvcf_region_table_parse_specs\(bvcf_region_table \*t, const char \*text, size_t n, int exclude, char \*err, size_t err_cap\);",
                 r"int bvcf_region_table_parse_bed\(bvcf_region_table \*t, const char \*text, size_t n, int exclude, char \*err, size_t err_cap\);",
                 r"int bvcf_region_table_build\(bvcf_region_table \*t\);", r"void bvcf_region_table_free\(bvcf_region_table \*t\);",
                 r"int bvcf_set_region_table\(bvcf_ctx \*ctx, const bvcf_region_table \*t\);",
                 r"void bvcf_region_gate_count\(const bvcf_result \*r, uint64_t out\[3\]\);",
                 r"void bvcf_config_regions_defaults\(bvcf_config_regions \*c\);"):
        assert re.search(decl, h), decl
    assert "#define BVCF_CONFIG_MORE_REGIONS 6\n" in h and bv.CONFIG_MORE_REGIONS == 6
    assert "#define BVCF_REGION_MAX_INTERVALS (1ull << 26)\n" in h and bv.REGION_MAX_INTERVALS == 1 << 26
    assert "#define BVCF_REGION_MAX_CHROMS (1ull << 20)\n" in h and bv.REGION_MAX_CHROMS == 1 << 20
    for name in ("bvcf_region_table_parse_specs", "bvcf_region_table_parse_bed", "bvcf_region_table_build", "bvcf_region_table_free",
                 "bvcf_region_table_has", "bvcf_region_table_stays", "bvcf_set_region_table", "bvcf_region_gate_count",
                 "bvcf_config_regions_defaults"):
        assert name in bv.EXPORTS and hasattr(bv.lib, name)
    for name in ("bvcf_bench_region_kernel", "bvcf_bench_region_gate_stride"):
        assert name in bv.BENCH_EXPORTS and hasattr(bv.lib, name)
    assert bv.REGION_REPORT == rg.REPORT
    assert bv.ABI_VERSION == 9 and bv.ABI_VERSION_SUBSET == 10


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    fields = ["regions", "regions_path", "exclude_regions", "exclude_regions_path", "region_filter_path"]
    tf = [f for f, _ in bv.RegionTableStruct._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu", sizeof(bvcf_config_variants), sizeof(bvcf_config_regions), sizeof(bvcf_region_table),'
                   "sizeof(bvcf_allele), offsetof(bvcf_allele, pad), sizeof(bvcf_line));"
                   + "".join('printf(" %%zu", offsetof(bvcf_config_regions, %s));' % f for f in fields)
                   + "".join('printf(" %%zu", offsetof(bvcf_region_table, %s));' % f for f in tf)
                   + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    G, T = bv.ConfigRegions, bv.RegionTableStruct
    assert out == [C.sizeof(bv.ConfigVariants), C.sizeof(G), C.sizeof(T), 64, 54, 64] + [getattr(G, f).offset for f in fields] + \
        [getattr(T, f).offset for f in tf]
    assert G.regions.offset == C.sizeof(bv.ConfigVariants) and G.variants.offset == 0
    assert bv.REGION_CHROM_DTYPE.itemsize == 32 and bv.REGION_INTERVAL_DTYPE.itemsize == 16


def test_older_defaults_write_what_they_wrote(bv):
    """each of the six older *_defaults leaves everything behind its own struct alone; the new one fills the whole struct"""
    G = bv.ConfigRegions
    older = ((bv.lib.bvcf_config_more_defaults, bv.ConfigMore.site_gate.offset, 0),
             (bv.lib.bvcf_config_gate_defaults, bv.ConfigMore.plink_prefix.offset, bv.CONFIG_MORE_GATE),
             (bv.lib.bvcf_config_plink_defaults, C.sizeof(bv.ConfigMore), bv.CONFIG_MORE_PLINK),
             (bv.lib.bvcf_config_trios_defaults, C.sizeof(bv.ConfigTrios), bv.CONFIG_MORE_TRIOS),
             (bv.lib.bvcf_config_ld_defaults, C.sizeof(bv.ConfigLd), bv.CONFIG_MORE_LD),
             (bv.lib.bvcf_config_variants_defaults, C.sizeof(bv.ConfigVariants), bv.CONFIG_MORE_VARIANTS))
    for fn, first_untouched, marker in older:
        g = G()
        C.memset(C.byref(g), 0xFF, C.sizeof(g))
        fn(C.byref(g))
        assert bytes(g)[first_untouched:] == b"\xff" * (C.sizeof(g) - first_untouched), fn
        base = g.variants.ld.trios.more.base
        assert base.reserved[0] == bv.CONFIG_MORE and base.reserved[1] == marker
    v = bv.ConfigVariants()
    bv.lib.bvcf_config_variants_defaults(C.byref(v))
    g = G()
    C.memset(C.byref(g), 0xFF, C.sizeof(g))
    bv.lib.bvcf_config_regions_defaults(C.byref(g))
    assert g.variants.ld.trios.more.base.reserved[1] == bv.CONFIG_MORE_REGIONS
    assert [g.regions, g.regions_path, g.exclude_regions, g.exclude_regions_path, g.region_filter_path] == [None] * 5
    assert (g.variants.keep_variants_path, g.variants.ld.ld_window) == (None, 50)
    g.variants.ld.trios.more.base.reserved[1] = bv.CONFIG_MORE_VARIANTS  # but for the marker, its head is what the older one makes
    assert bytes(g)[:C.sizeof(v)] == bytes(v)


def test_config_markers(bv):
    assert list(bv.make_config({"keepVariants": "/x"}).reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_VARIANTS]
    for key, field in bv.REGION_CONFIG_KEYS:
        c = bv.make_config({key: "chr1:5", "minMac": 3, "excludeVariants": "/l"})
        assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_REGIONS]
        g = C.cast(C.byref(c), C.POINTER(bv.ConfigRegions)).contents
        assert getattr(g, field) == b"chr1:5" and g.variants.ld.trios.more.site_gate.min_mac == 3 and g.variants.ld.ld_window == 50
        assert g.variants.exclude_variants_path == b"/l"
        assert [g.regions, g.regions_path, g.exclude_regions, g.exclude_regions_path, g.region_filter_path].count(None) == 4


# ---- the CLI's argument errors (no device is reached)

def cli(args, stdin_bytes=b""):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=60)


@pytest.mark.parametrize("flag", ["regions", "regionsFile", "excludeRegions", "excludeRegionsFile", "regionFilterReport"])
def test_cli_flag_without_a_value(flag):
    p = cli(["--" + flag])
    assert p.returncode == 2 and p.stdout == b""
    assert p.stderr == ("flag needs an argument: -%s\n" % flag).encode()


@pytest.mark.parametrize("flag", ["regions", "regionsFile", "excludeRegions", "excludeRegionsFile"])
def test_cli_empty_value(flag):
    p = cli(["--%s=" % flag])
    assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1
    assert ('invalid value "" for flag -%s: ' % flag).encode() in p.stderr


@pytest.mark.parametrize("flag", ["regions", "excludeRegions"])
@pytest.mark.parametrize("spec", ["chr1:200-100", "chr1,,chr2", ":5", "chr1,"])
def test_cli_bad_spec(flag, spec):
    p = cli(["--" + flag, spec], vl.rows_vcf(5))
    assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1
    assert ('invalid value "%s" for flag -%s: ' % (spec, flag)).encode() in p.stderr


@pytest.mark.parametrize("flag", ["regionsFile", "excludeRegionsFile"])
def test_cli_unreadable_bed(flag, tmp_path):
    """one message and exit code 1, before the input is looked at or a device asked for"""
    bad = tmp_path / "no_such_dir" / "r.bed"
    p = cli(["--" + flag, str(bad)], vl.rows_vcf(5))
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.count(b"\n") == 1 and str(bad).encode() in p.stderr and b"No such file" in p.stderr


@pytest.mark.parametrize("flag", ["regionsFile", "excludeRegionsFile"])
@pytest.mark.parametrize("text,line", [(b"chr1\t5\t9\nchr1\t9\n", 2), (b"#h\nchr1\t9\t5\n", 2), (b"chr1\tx\t5\n", 1), (b"chr1\t1\t" + b"1" * 19 + b"\n", 1)])
def test_cli_bad_bed_line(flag, text, line, tmp_path):
    bed = tmp_path / "bad.bed"
    bed.write_bytes(text)
    p = cli(["--" + flag, str(bed)], vl.rows_vcf(5))
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.count(b"\n") == 1
    assert str(bed).encode() in p.stderr and (b"line %d:" % line) in p.stderr


def test_cli_unwritable_report(tmp_path):
    bad = tmp_path / "no_such_dir" / "x.report"
    p = cli(["--regionFilterReport", str(bad)], vl.rows_vcf(5))
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.count(b"\n") == 1 and str(bad).encode() in p.stderr


def test_run_buffer_reports_a_bad_spec_before_any_device_work(bv):
    rc, out, log, _ = bv.run_buffer(vl.rows_vcf(5), {"regions": "chr1:9-1"})
    assert rc == bv.E_ARG and out == b"" and log.count("\n") == 1 and "regions: " in log


# ---- the conditions on the inputs of tests/test_gpu_regions.py, with the oracle alone

def oracle_body(vcf, cfg=None):
    rc, body, _, _ = orc.run(vcf, cfg or {})
    assert rc == 0
    return body


KINDS = (b"SNP", b"INS", b"DEL", b"MNP", b"MULTIALLELIC")


def keeps_and_drops(body, sets, kinds=()):
    mask = rg.select(body, sets)
    assert any(mask) and not all(mask), "regions that do not both keep and drop"
    for k in kinds:
        mine = [m for m, r in zip(mask, vl.rows_of(body)) if rg.kind_of(r) == k]
        assert any(mine) and not all(mine), k
    return mask


@pytest.mark.parametrize("ns", [1, 5])
def test_edges_input_keeps_and_drops_every_kind(ns):
    body = oracle_body(rg.edges_vcf(ns))
    assert {rg.kind_of(r) for r in vl.rows_of(body)} == set(KINDS)
    for sets in (rg.Sets(regions=rg.EDGE_KEEP), rg.Sets(exclude=rg.EDGE_KEEP), rg.Sets(regions=rg.EDGE_KEEP, exclude=rg.EDGE_EXCLUDE)):
        keeps_and_drops(body, sets, KINDS)
    rows = {(f[rg.POS], f[rg.ALT]): rg.Sets(regions=rg.EDGE_KEEP).row_stays(r) for r in vl.rows_of(body) for f in [r.split(b"\t")]}
    # what the edge rows are there for
    assert [rows[(p, b"T")] for p in (b"999", b"1000", b"2000", b"2001", b"2999", b"3000", b"3001", b"4999", b"5000")] == \
        [False, True, True, False, False, True, False, False, True]
    assert (rows[(b"995", b"-6")], rows[(b"995", b"-5")], rows[(b"2000", b"-10")], rows[(b"2001", b"-5")], rows[(b"2995", b"-10")],
            rows[(b"2995", b"-4")]) == (True, False, True, False, True, False)
    assert (rows[(b"2001", b"-1")], rows[(b"1000", b"-1")], rows[(b"1000", b"G")], rows[(b"2002", b"A")]) == (False, True, True, False)
    assert [rows[(p, b"+GG")] for p in (b"999", b"1000", b"2000", b"2001", b"3000")] == [False, True, True, False, True]
    assert [rows[(p, b"T")] for p in (b"0001500", b"007", b"1e3", b"+1500", b"", b"1234567890123456789", b"-1500", b"9" * 18, b"15OO", b"1500 ")] == \
        [True, False, False, False, False, False, False, True, False, False]
    assert rows[(b"1501", b"-1")]  # (POS "+1500" read by Atoi)
    # keep and exclude on one deletion that overlaps both sets: 2000 .. 2009 touches 1000-2000 and 2000-2001
    both = rg.Sets(regions=rg.EDGE_KEEP, exclude=rg.EDGE_EXCLUDE)
    assert rg.has_bits(both.keep, both.excl, b"chr7", b"2000", b"-10") == 3
    that = [r for r in vl.rows_of(body) if (r.split(b"\t")[rg.POS], r.split(b"\t")[rg.ALT]) == (b"2000", b"-10")]
    assert len(that) == 1 and not both.row_stays(that[0])


@pytest.mark.parametrize("ns", [1, 3])
def test_names_input_keeps_and_drops(ns):
    body = oracle_body(rg.names_vcf(ns))
    assert len(vl.rows_of(body)) == 3 * len(rg.NAMES)
    for sets in (rg.Sets(regions=rg.NAMES_KEEP), rg.Sets(exclude=rg.NAMES_EXCLUDE), rg.Sets(regions=rg.NAMES_KEEP, exclude=rg.NAMES_EXCLUDE)):
        keeps_and_drops(body, sets)
    mask = rg.select(body, rg.Sets(regions=rg.NAMES_KEEP, exclude=rg.NAMES_EXCLUDE))
    by_name = {nm: mask[3 * i:3 * i + 3] for i, nm in enumerate(rg.NAMES)}
    assert by_name["1"] == by_name["chr1"] == [True, False, True] and by_name["chr10"] == by_name["10"] == [False, True, False]
    assert by_name["M"] == by_name["chrM"] == [True] * 3 and by_name["chrom"] == [False] * 3 and by_name["c"] == [True] * 3
    assert by_name["cat"] == [True, True, False] and by_name["chrUn_gl000220_random"] == [True, True, False]
    assert by_name["HLA:DRB1"] == [True] * 3 and by_name["ctg:5"] == [True, True, False] and by_name["ctg"] == [False] * 3
    assert by_name["X"] == by_name["2"] == by_name["3"] == [False] * 3
    only_x = rg.select(body, rg.Sets(exclude=rg.NAMES_EXCLUDE))
    assert [only_x[3 * i:3 * i + 3] for i, nm in enumerate(rg.NAMES) if nm in ("X", "2")] == [[False] * 3, [True] * 3]


def test_counts_input_has_rows_around_every_interval():
    vcf, bed = rg.counts_vcf_and_bed()
    body = oracle_body(vcf)
    iv = rg.parse_bed(bed)
    assert sorted(len(v) for v in rg.merged(iv).values()) == sorted(n for n in rg.COUNTS if n)
    for sets in (rg.Sets(regions_bed=bed), rg.Sets(exclude_bed=bed)):
        mask = keeps_and_drops(body, sets, (b"SNP", b"DEL"))
    rows = [r.split(b"\t") for r in vl.rows_of(body)]
    assert 300 < len(rows) < 600
    for c, b, e in iv:  # both edges and both neighbours of every interval, and a row in the gap behind it
        have = {int(f[rg.POS]) for f in rows if f[rg.CHROM] == c and f[rg.ALT] == b"T"}
        assert {b - 1, b, e, e + 1, e + 40} <= have
    assert not any(m for m, f in zip(rg.select(body, rg.Sets(regions_bed=bed)), rows) if f[rg.CHROM] == b"chrn0")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_run_shape_inputs(n):
    body = oracle_body(vl.rows_vcf(n))
    assert len(vl.rows_of(body)) == n
    if n > 1:
        keeps_and_drops(body, rg.rows_sets(n))
    else:
        assert rg.select(body, rg.rows_sets(1)) == [True]


def test_wrap_input_keeps_and_drops(bv):
    listed, every = rg.wrap_case(bv)
    mask = keeps_and_drops(oracle_body(rg.ctg_vcf(every)), rg.Sets(regions=b",".join(rg.ctg(i) for i in listed)))
    assert mask == [i in listed for i in every]


def test_composition_inputs_keep_and_drop():
    for vcf in (sg.case_input("sweep"), sg.case_input("fuzz13"), sg.case_input("masked13"), sg.case_input("rare300"),
                sg.case_input("cut300"), vl.pedigree_case()[0], vl.round_trip_input()[0]):
        body = oracle_body(vcf)
        keeps_and_drops(body, rg.half_sets(body))


def test_golden_sets_keep_and_drop():
    vcf = gzip.decompress(open(GOLDEN_GZ, "rb").read())
    body = oracle_body(vcf)
    third, bed = rg.golden_sets(body)
    n = len(vl.rows_of(body))
    m = keeps_and_drops(body, third)
    assert n // 6 < sum(m) < n // 2
    m = keeps_and_drops(body, bed)
    assert n // 2 < sum(m) < n and rg.n_merged(bed.excl) == 300
