"""The inputs of closed_domains.py hold what test_gpu_closed_domains.py needs them to hold -- shown with the oracle alone.

These are conditions on the inputs, not measurements: when one fails the input is changed, never the bound."""
import collections
import re

import pytest

import closed_domains as cd
import oracle_lib as orc

HET, HOM, MISSING, IDX = 6, 8, 10, 15  # columns of a row with keepInfo (parse.Header, then alleleIdx and info)


def rows_of(vcf, cfg=None):
    rc, out, log, n = orc.run(vcf, cfg)
    assert rc == 0 and n == vcf.count(b"\n") - 3  # (two meta lines and the header line)
    return [r.split(b"\t") for r in out.split(b"\n")[:-1]], log


def test_probe_sets_have_the_stated_sizes():
    assert len(cd.g3_probes()) == 6044 and len(set(cd.g3_probes())) == 6044
    assert sum(cd.is_regular(p) for p in cd.g3_probes()) == 242
    assert all(len(p) == 3 and p[1] in b"|/" and 0x09 not in p and 0x0A not in p for p in cd.g3_probes())
    assert {p[0] for p in cd.g3_probes()} == set(range(256)) - {0x09, 0x0A}
    square = cd.g3_square()
    assert len(square) == 2 * 32 * 32 and sum(cd.is_regular(p) for p in square) == 242
    assert len(cd.gg_probes()) == 2801 + 3125 == len(set(cd.gg_probes()))
    for s in (b"10|11", b"01|10", b"1|1|1", b"1||1", b"./.|.", b"", b".", b"0:1", b"2/2"):
        assert s in cd.gg_probes()
    assert (len(cd.r_single()), len(cd.r_pairs()), len(cd.r_wordsize())) == (2346, 6762, 5040)
    assert len(cd.r_records("rowedge")) == 300 * 27 and len(cd.r_records("chrom")) == 1365
    assert len(cd.r_records("pos")) == len(cd.R_POS) * len(cd.R_POS_PAIRS) == 300
    assert len(set(cd.r_first_three())) == 14148


def test_inputs_have_the_stated_shape():
    g3 = cd.g3("list") + cd.g3("dense")
    assert 13.0e6 < len(g3) < 13.5e6
    for vcf, ns in ((cd.g3("list"), 260), (cd.g3("dense"), 260), (cd.g3_last("lf"), 260), (cd.g3_many(2600, "raw"), 2600),
                    (cd.g3_many(2500, "dense"), 2500),
                    (cd.gg("gt"), 68), (cd.gg("gtdpgq", True), 68)):
        lines = vcf.split(b"\n")[2:-1]
        assert {ln.count(b"\t") for ln in lines} == {8 + ns}
    assert cd.g3("list").count(b"\n") - 3 == 6044 and cd.gg("gt").count(b"\n") + cd.gg("gtdpgq").count(b"\n") - 6 == 11852
    assert 5.5e6 < len(cd.gg("gt")) + len(cd.gg("gtdpgq")) < 5.7e6
    assert cd.g3_last("crlf").count(b"\r\n") == cd.g3_last("crlf").count(b"\n") == cd.g3_last("lf").count(b"\n")
    # a piece in parts is the piece: every line once, as it is in the whole
    whole = cd.piece("g3_2500-raw")
    assert b"".join(cd.piece("g3_2500-raw-part%dof4" % k).split(b"\n", 3)[3] for k in range(4)) == whole.split(b"\n", 3)[3]
    assert all(cd.piece("g3_2500-raw-part%dof4" % k).split(b"\n", 3)[:3] == whole.split(b"\n", 3)[:3] for k in range(4))
    # the probe is where g3_probe_at says, the carriers in front, and every probe position 8..259 is used
    for i, p in list(enumerate(cd.g3_probes()))[::97]:
        f = cd.g3("dense").split(b"\n")[3 + i].split(b"\t")[9:]
        assert f[cd.g3_probe_at(i)] == p and f[0][::2] == b"12" and f[4][::2] == b"99"
    assert {cd.g3_probe_at(i) for i in range(6044)} == set(range(8, 260))
    # the densities: list mode stays below a class list's 15 map bytes, the raw list takes 16..63 lanes (4 samples each), all
    # distinct, dense more than 63 -- at 2 600 samples also more than 63 lanes with a digit >= 2
    def lanes(vcf, k, only_high=False):
        f = vcf.split(b"\n")[3 + k].split(b"\t")[9:]
        ref = b"0" + f[100][1:2] + b"0"
        return {s // 4 for s, x in enumerate(f) if x != ref and (not only_high or set(x[::2]) - set(b"01"))}
    for k in (0, 500, 2047):
        assert len(lanes(cd.g3("list"), k)) <= 3 and len(lanes(cd.g3("dense"), k)) > 63
        for ns in cd.G3_MANY_SAMPLES:
            assert len(lanes(cd.g3_many(ns, "list"), k)) <= 3 and 16 <= len(lanes(cd.g3_many(ns, "raw"), k)) <= 63
            assert len(lanes(cd.g3_many(ns, "dense"), k)) > 63 and len(lanes(cd.g3_many(ns, "dense"), k, True)) > 63
            assert len(lanes(cd.g3_many(ns, "raw"), k, True)) <= 3


def _check_every_line_has_a_row(vcf):
    rows, _ = rows_of(vcf)
    seen = {r[1] for r in rows}
    want = {ln.split(b"\t", 2)[1] for ln in vcf.split(b"\n")[3:-1]}
    assert len(want) == vcf.count(b"\n") - 3  # (POS names the line)
    assert want <= seen, sorted(want - seen)[:5]


@pytest.mark.parametrize("piece", ["g3-list", "g3-dense", "g3_last-lf", "g3_last-crlf", "g3_2600-list", "g3_2600-raw", "g3_2600-dense",
                                   "g3_2500-list", "g3_2500-raw", "g3_2500-dense",
                                   "gg-gt", "gg-gtdpgq", "gg-gt-last", "gg-gtdpgq-last"])
def test_every_line_yields_a_row(piece):
    _check_every_line_has_a_row(cd.piece(piece))


def _probe_classes(vcf, probe_at):
    """ALT indices at which the probe sample of a line is het / hom / missing / none, over the oracle's rows"""
    rows, _ = rows_of(vcf, {"keepInfo": True})
    seen = {"het": set(), "hom": set(), "missing": set(), "none": set()}
    for r in rows:
        name = b"S%05d" % probe_at(int(r[1]) - 1000)
        where = [k for k, col in (("het", HET), ("hom", HOM), ("missing", MISSING)) if name in r[col].split(b";")]
        assert len(where) <= 1
        seen[where[0] if where else "none"].add(int(r[IDX]))
    return seen


def test_probe_sample_is_seen_in_every_class():
    g3 = collections.defaultdict(set)
    for d in cd.G3_DENSITIES:
        for k, v in _probe_classes(cd.g3(d), cd.g3_probe_at).items():
            g3[k] |= v
    gg = collections.defaultdict(set)
    for form in cd.GG_FORMS:
        for k, v in _probe_classes(cd.gg(form), cd.gg_probe_at).items():
            gg[k] |= v
    for seen in (g3, gg):
        for k in ("het", "hom", "missing", "none"):
            assert len(seen[k]) >= 3, (k, sorted(seen[k]))
    # (every ALT of the lists is valid next to one of the four REFs: every ALT index has rows)
    assert g3["none"] == set(range(9)) and gg["none"] == set(range(11))


MESSAGES = [r" : REF == ALT$", r" ALT #1 ALT not ACTG$", r" ALT #1 empty REF$", r" ALT #1 1st base REF != ALT$", r" ALT #1 Invalid POS$",
            r"^\S* empty REF$", r" ALT #[2-9] ALT not ACTG$", r" ALT #\d+ 1st base ALT != REF$", r"^\S* Invalid POS$",
            r" ALT#\d+ 1st base REF != ALT$", r" ALT#\d+ Mixed indel/snp sites not supported$"]


def test_r_holds_every_record_type_and_every_message():
    types, log = collections.Counter(), []
    for block in ("single", "pairs", "wordsize"):
        rows, lg = rows_of(cd.r(block))
        types.update(r[2] for r in rows)
        log += lg.split("\n")
    log += rows_of(cd.r("pos"))[1].split("\n")
    assert types == {b"SNP": 512, b"INS": 1676, b"DEL": 445, b"MNP": 1496, b"MULTIALLELIC": 5903}
    for m in MESSAGES:
        assert any(re.search(m, ln) for ln in log), m
    # sites-only, and with 70 samples (lines long enough for k_order's fast lane): the same rows
    assert len(rows_of(cd.r("pairs", samples=0))[0]) == 5903 == len(rows_of(cd.r("pairs", samples=cd.R_LONG_SAMPLES))[0])
    assert min(len(ln) for blk in cd.R_BLOCKS for ln in cd.r(blk, cd.R_LONG_SAMPLES).split(b"\n")[3:-1]) >= 256 + 3
    # the row edge: REF starts at every offset from 24 bytes before the end of the staged head to 2 bytes past it
    offs = collections.Counter(len(b"\t".join(rec[:3])) + 1 for rec in cd.r_records("rowedge"))
    assert offs == {o: 300 for o in range(cd.HEAD_ROW_BYTES - 24, cd.HEAD_ROW_BYTES + 3)}
    assert {r[2] for r in rows_of(cd.r("rowedge"))[0]} == set(types)
    assert len(rows_of(cd.r("chrom"))[0]) == 1365


def test_wrapping_pos_rows_are_in_the_oracle_output():
    rows, log = rows_of(cd.r("pos"))
    at = {(r[0], r[1]) for r in rows}
    for pos in cd.R_POS_WRAPS:
        k = cd.R_POS.index(pos)
        for pair in cd.R_POS_WRAP_PAIRS:
            assert (cd.r_pos_chrom(k, cd.R_POS_PAIRS.index(pair)), b"-9223372036854775808") in at, (pos, pair)
    # ... and the neighbours that do not wrap, the tenth digit, the leading zeros
    k = cd.R_POS.index(b"9223372036854775806")
    assert (cd.r_pos_chrom(k, 1), b"9223372036854775807") in at
    assert (cd.r_pos_chrom(cd.R_POS.index(b"1000000000"), 1), b"1000000001") in at
    assert (cd.r_pos_chrom(cd.R_POS.index(b"1234567890"), 6), b"1234567891") in at
    assert (cd.r_pos_chrom(cd.R_POS.index(b"00000000000000000000123"), 1), b"124") in at
    assert (cd.r_pos_chrom(cd.R_POS.index(b"-9223372036854775808"), 1), b"-9223372036854775807") in at
    assert log.count("Invalid POS") > 50
