"""--regions / --excludeRegions: the expected selection, written from the rules in include/bvcf.h (bvcf_region_table), not
from the kernel: a SPEC parser, a BED parser, the span of a row from its TSV columns pos and alt, and a naive "any interval
overlaps" test over the intervals as given -- the selection sorts and merges nothing (merged() and painted() are the
references of the table's merging and of the report's interval counts).

select() decides every row of an oracle run; the expected TSV is the oracle's with the unselected rows taken out, every
other expected output is the reference of its own module over the rows that stay.  The inputs of
tests/test_gpu_regions.py are made here.  Test infrastructure only."""
import functools
import re

import vcfgen
import variantlist as vl
from pairtable import BASE_HEADER

REPORT = ["keepIntervals", "excludeIntervals", "examined", "kept", "dropped"]
CHROM, POS, ALT = (BASE_HEADER.index(x) for x in ("chrom", "pos", "alt"))
MAX_COORD = (1 << 63) - 1
_D = re.compile(rb"[0-9]{1,18}\Z")
_POS = re.compile(rb"-?[0-9]{1,18}\Z")


class SpecError(ValueError):
    pass


class BedError(ValueError):
    def __init__(self, line_no, what):
        super().__init__("line %d: %s" % (line_no, what))
        self.line_no = line_no


def norm(name):
    """the TSV's rule for CHROM: "chr" in front unless the name has four bytes or more and starts with 'c'"""
    return name if len(name) >= 4 and name[:1] == b"c" else b"chr" + name


def _d(s):
    return int(s) if _D.match(s) and int(s) >= 1 else None


def parse_spec(spec):
    """one SPEC -> (normalised chrom, beg, end)"""
    if not spec:
        raise SpecError("an empty SPEC")
    chrom, beg, end = spec, 1, MAX_COORD
    if b":" in spec:
        head, tail = spec.rsplit(b":", 1)
        got = None
        if b"-" not in tail:
            if _d(tail) is not None:
                got = (_d(tail), _d(tail))
        else:
            b, e = tail.split(b"-", 1)
            if _d(b) is not None and (e == b"" or _d(e) is not None):
                got = (_d(b), MAX_COORD if e == b"" else _d(e))
        if got is not None:
            chrom, (beg, end) = head, got
            if beg > end:
                raise SpecError("BEG > END")
    if not chrom:
        raise SpecError("an empty CHROM")
    return norm(chrom), beg, end


def parse_specs(text):
    return [parse_spec(s) for s in text.split(b",")]


def parse_bed(text):
    """the intervals of a BED text, 1-based inclusive, as given"""
    out = []
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for no, ln in enumerate(lines, 1):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln or ln.startswith((b"#", b"track", b"browser")):
            continue
        f = ln.split(b"\t")
        if len(f) < 3:
            raise BedError(no, "fewer than three columns")
        if not _D.match(f[1]) or not _D.match(f[2]):
            raise BedError(no, "start or end is not 1 to 18 digits")
        s, e = int(f[1]), int(f[2])
        if s > e:
            raise BedError(no, "start > end")
        if s == e:
            continue
        out.append((norm(f[0]), s + 1, e))
    return out


def pos_of(text):
    """the TSV's pos column as a position, or None"""
    return int(text) if _POS.match(text) else None


def span(pos_text, alt):
    p = pos_of(pos_text)
    if p is None:
        return None
    if alt.startswith(b"-") and alt[1:].isdigit():
        return p, p + max(int(alt[1:]), 1) - 1
    return p, p


def overlaps(intervals, chrom, sp):
    """naive: any interval of the chromosome shares a base with the span"""
    return sp is not None and any(c == chrom and b <= sp[1] and e >= sp[0] for c, b, e in intervals)


def stays(keep, exclude, chrom, pos_text, alt):
    """keep: the intervals of the keep set, or None when no keep flag was given; exclude: those of the exclude set"""
    sp = span(pos_text, alt)
    return (keep is None or overlaps(keep, chrom, sp)) and not overlaps(exclude or [], chrom, sp)


def has_bits(keep, exclude, chrom, pos_text, alt):
    sp = span(pos_text, alt)
    return (1 if overlaps(keep or [], chrom, sp) else 0) | (2 if overlaps(exclude or [], chrom, sp) else 0)


def merged(intervals):
    """{chrom: [(beg, end), ...]}: sorted, overlapping and abutting intervals made one"""
    out = {}
    for c, b, e in sorted(intervals):
        mine = out.setdefault(c, [])
        if mine and b <= mine[-1][1] + 1:
            mine[-1] = (mine[-1][0], max(mine[-1][1], e))
        else:
            mine.append((b, e))
    return out


def painted(intervals, limit):
    """the same by painting the bases 1 .. limit of every chromosome and reading the runs off (small coordinates only)"""
    out = {}
    for c in {c for c, _, _ in intervals}:
        bases = [False] * (limit + 2)
        for cc, b, e in intervals:
            if cc == c:
                for x in range(b, min(e, limit) + 1):
                    bases[x] = True
        runs, x = [], 1
        while x <= limit:
            if bases[x]:
                y = x
                while bases[y + 1]:
                    y += 1
                runs.append((x, y))
                x = y + 1
            x += 1
        out[c] = runs
    return out


def n_merged(intervals):
    return sum(len(v) for v in merged(intervals).values())


class Sets:
    """the four flags of one run: SPEC texts and BED texts (bytes or None)"""

    def __init__(self, regions=None, regions_bed=None, exclude=None, exclude_bed=None):
        self.regions, self.regions_bed, self.exclude, self.exclude_bed = regions, regions_bed, exclude, exclude_bed
        self.keep = None
        if regions is not None or regions_bed is not None:
            self.keep = (parse_specs(regions) if regions is not None else []) + (parse_bed(regions_bed) if regions_bed is not None else [])
        self.excl = (parse_specs(exclude) if exclude is not None else []) + (parse_bed(exclude_bed) if exclude_bed is not None else [])

    def key(self):
        return (self.regions, self.regions_bed, self.exclude, self.exclude_bed)

    def table(self, bv):
        return bv.RegionTable(keep=self.regions, keep_bed=self.regions_bed, exclude=self.exclude, exclude_bed=self.exclude_bed)

    def cfg(self, tmp_path, tag="r"):
        """the run_buffer / CLI keys; BED texts are written under tmp_path"""
        out = {}
        if self.regions is not None:
            out["regions"] = self.regions.decode()
        if self.exclude is not None:
            out["excludeRegions"] = self.exclude.decode()
        for key, text in (("regionsFile", self.regions_bed), ("excludeRegionsFile", self.exclude_bed)):
            if text is not None:
                p = tmp_path / ("%s.%s.bed" % (tag, key))
                p.write_bytes(text)
                out[key] = str(p)
        return out

    def cli_args(self, tmp_path, tag="r"):
        out = []
        for k, v in self.cfg(tmp_path, tag).items():
            out += ["--" + k, v]
        return out

    def row_stays(self, row):
        f = row.split(b"\t")
        return stays(self.keep, self.excl, f[CHROM], f[POS], f[ALT])

    def report(self, c):
        v = [n_merged(self.keep or []), n_merged(self.excl)] + list(c)
        return "".join("%s\t%d\n" % (nm, x) for nm, x in zip(REPORT, v)).encode()


def select(tsv_body, sets, has_samples=True):
    """-> the mask of a TSV body (no header line): True for the rows that stay.  A file without sample columns comes out
    unchanged"""
    return [(not has_samples) or sets.row_stays(r) for r in vl.rows_of(tsv_body)]


def bed_text(intervals, eol=b"\n"):
    """1-based inclusive (chrom, beg, end) as BED lines"""
    return b"".join(b"%s\t%d\t%d%s" % (c, b - 1, e, eol) for c, b, e in intervals)


def kind_of(row):
    f = row.split(b"\t")
    return f[BASE_HEADER.index("type")]


# ---- inputs

_line = vl._line


@functools.lru_cache(maxsize=None)
def edges_vcf(ns):
    """chromosome 7 (written without "chr"), to be read with EDGE_KEEP = 1000-2000, 3000, 5000- : SNPs at beg - 1, beg,
    end, end + 1 of each; deletions that touch an interval with their first or their last base only, end one base short,
    start one base late, or cover a whole interval that lies strictly inside them; multiallelic lines whose SNP row and
    deletion row, one base apart, fall on different sides; MNPs of which one base is in; insertions at the edges; POS texts
    that are positions in disguise (leading zeros) or no positions at all; 18 digits"""
    out = [vcfgen.header(ns)]
    for p in (999, 1000, 1500, 2000, 2001, 2999, 3000, 3001, 4999, 5000, 6000):
        out.append(_line("7", p, "A", "T", ns))
    out.append(_line("7", 994, "ACGTACG", "A", ns))         # -6 at 995: 995 .. 1000, the last base touches
    out.append(_line("7", 994, "ACGTAC", "A", ns))          # -5 at 995: 995 .. 999, one base short
    out.append(_line("7", 1999, "ACGTACGTACG", "A", ns))    # -10 at 2000: the first base touches
    out.append(_line("7", 2000, "ACGTAC", "A", ns))         # -5 at 2001: one base late
    out.append(_line("7", 2994, "ACGTACGTACG", "A", ns))    # -10 at 2995: 2995 .. 3004 covers 3000
    out.append(_line("7", 2994, "ACGTA", "A", ns))          # -4 at 2995: 2995 .. 2998, short of 3000
    out.append(_line("7", 4000, "ACG", "A", ns))            # -2 at 4001: in a gap
    out.append(_line("7", 2000, "AC", "TC,A", ns))          # the SNP row at 2000 is in, the deletion at 2001 is out
    out.append(_line("7", 999, "AC", "TC,A", ns))           # the reverse: 999 out, the deletion at 1000 in
    out.append(_line("7", 999, "AC", "TG", ns))             # an MNP: 999 out, 1000 in
    out.append(_line("7", 2000, "ACG", "TCA", ns))          # an MNP: 2000 in, 2002 out
    out.append(_line("7", 4999, "AC", "TG", ns))
    for p in (999, 1000, 2000, 2001):
        out.append(_line("7", p, "A", "AGG", ns))           # insertions at their anchors
    out.append(_line("7", 2999, "AT", "ATGG", ns))          # an insertion k_head places: its anchor is 3000
    for p in ("0001500", "007", "1e3", "+1500", "", "1234567890123456789", "-1500", "999999999999999999", "15OO", "1500 "):
        out.append(_line("7", p, "A", "T", ns))
    out.append(_line("7", "+1500", "AC", "A", ns))          # Atoi reads +1500: the deletion's pos is printed as 1501
    return "".join(out).encode()


EDGE_KEEP = b"7:1000-2000,chr7:3000,7:5000-"
EDGE_EXCLUDE = b"chr7:1400-1600,7:2000-2001,7:6000"


@functools.lru_cache(maxsize=None)
def names_vcf(ns):
    """chromosome names: `1` against `chr1` (one chromosome), `chr1` against `chr10`, `M` and `chrM`, names that keep their
    own form (`chrom`, `c`, `cat`), a contig longer than 7 bytes, names containing ':'; three rows each, at 100, 200, 300"""
    out = [vcfgen.header(ns)]
    for ch in NAMES:
        for p in (100, 200, 300):
            out.append(_line(ch, p, "A", "T", ns))
    return "".join(out).encode()


NAMES = ["1", "chr1", "chr10", "10", "M", "chrM", "chrom", "c", "cat", "chrUn_gl000220_random", "HLA:DRB1", "ctg:5", "ctg", "X", "2", "3"]
# keep: chr1 by its short name, chr10 at 200 only, chrM whole, the long contig, the name with ':' whole and the other one
# through its last ':', and `ctg:5` as CHROM:POS -- position 5 of `ctg`, which no row has; exclude: chr1 at 200, X whole (a
# chromosome with exclude intervals only), chrcat; `2` and `3` are in neither set
NAMES_KEEP = b"1,chr10:200,M,chrUn_gl000220_random:100-250,HLA:DRB1,ctg:5:100-200,ctg:5,c,cat"
NAMES_EXCLUDE = b"chr1:200,X,chrcat:300-"


def counts_vcf_and_bed(ns=2):
    """chromosomes n0, n1, ... with 0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17 intervals [100 j + 10, 100 j + 20], j = 1 .. n, and
    rows before the first, at both edges and one base outside them, between each pair and after the last"""
    out, iv = [vcfgen.header(ns)], []
    for n in COUNTS:
        ch = "n%d" % n
        out.append(_line(ch, 50, "A", "T", ns))
        for j in range(1, n + 1):
            iv.append((("chr" + ch).encode(), 100 * j + 10, 100 * j + 20))
            for p in (100 * j + 9, 100 * j + 10, 100 * j + 20, 100 * j + 21, 100 * j + 60):
                out.append(_line(ch, p, "A", "T", ns))
        out.append(_line(ch, 100 * (n + 1) + 15, "A", "T", ns))
        out.append(_line(ch, 100 * n + 11, "ACGTACGTACGTACGT", "A", ns))  # -15 from 100 n + 12: over the last interval's end
    # (given out of order: the table sorts)
    return "".join(out).encode(), bed_text(iv[1::2] + iv[0::2])


COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]


def sites_vcf(n):
    """n lines without FORMAT and sample columns on chromosomes 1, 2 and 3: SNPs, every third line multiallelic"""
    out = [vcfgen.header(0, with_format=False)]
    for i in range(n):
        out.append("\t".join(["%d" % (1 + i % 3), str(1000 + i), ".", "A", "C,G" if i % 3 == 0 else "T", "50", "PASS", "."]) + "\n")
    return "".join(out).encode()


def rows_sets(n):
    """for vl.rows_vcf(n) -- rows chr1 / chr2 / chr3 in turn at 1000 + i: chr1 whole and a third of the span of chr2"""
    return Sets(regions=b"1,chr2:%d-%d" % (1000 + n // 3, 1000 + 2 * n // 3))


# ---- crafted name tables: contigs "ctg<i>_random" placed by the exported hash

def ctg(i):
    return b"ctg%d_random" % i


_PAIR = {}


def collision_pair(bv, capacity=16, limit=1 << 21):
    """the first two contigs ctg<p>, ctg<q> whose names agree in tag (h >> 32) and home slot at `capacity`"""
    if capacity not in _PAIR:
        h_of, seen = vl._hasher(bv), {}
        for i in range(1, limit):
            s = ctg(i)
            h = h_of(s, len(s))
            key = (h >> 32, h & (capacity - 1))
            if key in seen:
                _PAIR[capacity] = (seen[key], i)
                break
            seen[key] = i
        else:
            raise AssertionError("no pair below %d" % limit)
    return _PAIR[capacity]


def home_slot_ctgs(bv, slot, count, capacity=16, start=1):
    h_of, out, i = vl._hasher(bv), [], start
    while len(out) < count:
        s = ctg(i)
        if h_of(s, len(s)) & (capacity - 1) == slot:
            out.append(i)
        i += 1
    return out


def ctg_vcf(ids, ns=2):
    """one carried SNP row at 100 per contig"""
    return (vcfgen.header(ns) + "".join(_line(ctg(i).decode(), 100, "A", "T", ns, ["0|1"] * ns) for i in ids)).encode()


def wrap_case(bv):
    """(contigs in the table, all contigs of the file): four names with home slot 15 of 16 -- the probe chain runs 15, 0, 1,
    2 --, and in the file also names of home slots 15, 0 and 3 that are not in the table and walk the chain to its end"""
    listed = home_slot_ctgs(bv, 15, 4)
    others = home_slot_ctgs(bv, 15, 2, start=listed[-1] + 1) + home_slot_ctgs(bv, 0, 2) + home_slot_ctgs(bv, 3, 2)
    return listed, sorted(set(listed + others))


def collision_case(bv):
    """(contigs in the table, contigs of the file): the table holds A and C, the file B (A's partner in tag and home slot), C
    and D"""
    a, b = collision_pair(bv)
    c, d = [i for i in range(1, 10) if i not in (a, b)][:2]
    return [a, c], sorted([b, c, d])


def half_sets(body):
    """regions that keep about half of any body: every chromosome from the median of its positions on"""
    by = {}
    for r in vl.rows_of(body):
        f = r.split(b"\t")
        if pos_of(f[POS]) is not None:
            by.setdefault(f[CHROM], []).append(pos_of(f[POS]))
    return Sets(regions=b",".join(b"%s:%d-" % (c, max(sorted(ps)[len(ps) // 2], 1)) for c, ps in sorted(by.items())))


def kept_loci(body, mask):
    """the locus strings of the rows that stay: the list of the --keepVariants run that must agree with the region run"""
    return sorted({vl.locus(r) for r, m in zip(vl.rows_of(body), mask) if m})


def golden_span(body):
    """(lo, hi) of the positions of a TSV body"""
    ps = [pos_of(r.split(b"\t")[POS]) for r in vl.rows_of(body)]
    ps = [p for p in ps if p is not None]
    return min(ps), max(ps)


def golden_sets(body):
    """the two runs over the 1KG slice: the middle third of its span as a SPEC; an exclude BED of 300 small intervals"""
    lo, hi = golden_span(body)
    w = (hi - lo) // 3
    step = (hi - lo) // 300
    chrom = vl.rows_of(body)[0].split(b"\t")[CHROM]
    bed = bed_text([(chrom, lo + j * step, lo + j * step + step // 4) for j in range(300)])
    return Sets(regions=b"%s:%d-%d" % (chrom[3:], lo + w, lo + 2 * w)), Sets(exclude_bed=bed)
