"""--keepVariants / --excludeVariants: the expected selection, written from the definitions in include/bvcf.h
(bvcf_set_variant_list), not from the kernel.

A row's locus string is made from the oracle TSV's chrom, pos, ref and alt columns joined by ':'.  select() decides every
row of an oracle run; the expected TSV is the oracle's with the unselected rows taken out, every other expected output is
the reference of its own module over the rows that stay (sitegate.gate for a site gate behind the list).  The inputs of
tests/test_gpu_variant_list.py are made here, and the collision search, which works through the hash and the capacity
rule the library exports.  Test infrastructure only."""
import ctypes as C
import functools
import random

import vcfgen
from pairtable import BASE_HEADER

REPORT = ["listed", "examined", "kept", "dropped"]
COLS = [BASE_HEADER.index(x) for x in ("chrom", "pos", "ref", "alt")]


def rows_of(tsv_body):
    return [r for r in tsv_body.split(b"\n") if r]


def locus(row):
    f = row.split(b"\t")
    return b":".join(f[c] for c in COLS)


def loci_of(tsv_body):
    return [locus(r) for r in rows_of(tsv_body)]


def select(tsv_body, loci, exclude, has_samples=True):
    """-> the mask of a TSV body (no header line): True for the rows that stay.  A file without sample columns comes out
    unchanged"""
    want = set(loci)
    return [(not has_samples) or ((locus(r) in want) != bool(exclude)) for r in rows_of(tsv_body)]


def counts(mask, has_samples=True):
    """examined, kept, dropped: every row of a file with samples is an examined row"""
    return [len(mask), sum(mask), len(mask) - sum(mask)] if has_samples else [0, 0, 0]


def report_text(n_listed, c):
    return "".join("%s\t%d\n" % (nm, v) for nm, v in zip(REPORT, [n_listed] + list(c))).encode()


def list_text(loci, eol=b"\n"):
    return b"".join(x + eol for x in loci)


def parse_list(text):
    """the entries of a list file by the rules of include/bvcf.h: split at '\\n', one trailing '\\r' dropped, empty lines
    ignored, nothing trimmed; in order, duplicates included"""
    out = []
    for ln in text.split(b"\n"):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if ln:
            out.append(ln)
    return out


def fnv1a64(s):
    """FNV-1a, 64 bits, as include/bvcf.h states it (the CPU tests hold bvcf_locus_hash against this)"""
    h = 0xcbf29ce484222325
    for b in s:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def capacity_rule(n):
    cap = 16
    while cap < 2 * n:
        cap *= 2
    return cap


# ---- inputs

# genotypes by the number of ALTs: five samples carry every ALT; one sample carries two at most, so that a line with three
# has an ALT no sample carries (no row, and nothing examined)
GTS = {1: ["0|1", "1|1", "0|0", "./.", "1|0"], 2: ["1|2", "0|2", "0|1", "1|1", "2|2"], 3: ["1|2", "3|0", "0|1", "1|1", "2|3"]}


def _line(chrom, pos, ref, alt, ns, gts=None):
    gts = gts or [GTS[alt.count(",") + 1][s % 5] for s in range(ns)]
    return "\t".join([chrom, str(pos), ".", ref, alt, "50", "PASS", ".", "GT"] + gts) + "\n"


INS_LENGTHS = [1, 7, 8, 9, 300]
DEL_LENGTHS = [1, 9, 10, 123]
CHROMS = ["1", "chr1", "c", "cat", "chrom", "X", "chrUn_gl000220"]


@functools.lru_cache(maxsize=None)
def kinds_vcf(ns):
    """every kind of row in one small file: SNPs on every kind of CHROM (`1` and `chr1` give the same locus twice), a POS
    with leading zeros (printed as it stands), multiallelic lines, an MNP, insertions and deletions whose lengths change
    the digit count, and -- with one sample -- ALTs no sample carries (rows that are not examined)"""
    rng = random.Random(9300 + ns)
    out = [vcfgen.header(ns)]
    for ch in CHROMS:
        out.append(_line(ch, 100, "A", "T", ns))
        out.append(_line(ch, 1000, "A", "T", ns))
    out.append(_line("chr1", "00100", "A", "T", ns))       # the POS bytes verbatim: "chr1:00100:A:T"
    out.append(_line("chr1", 100, "A", "C", ns))
    out.append(_line("chr1", 100, "G", "T", ns))
    out.append(_line("chr2", 200, "A", "C,G,T", ns))        # three rows, two in the extra slots
    out.append(_line("chr2", 300, "ACG", "TCA", ns))        # MNP: rows at 300 and 302
    for n in INS_LENGTHS:
        out.append(_line("chr3", 1000 + n, "A", "A" + vcfgen.rand_bases(rng, n), ns))
    out.append(_line("chr3", 2000, "A", "AAC,AACG", ns))    # +AC and +ACG at one position
    for n in DEL_LENGTHS:
        out.append(_line("chr4", 3000 + 200 * n, "A" + vcfgen.rand_bases(rng, n), "A", ns))
    out.append(_line("chr4", 9000, "ACGTACGTAC", "A,AC,ACG", ns))  # -9, -8, -7 at neighbouring positions
    out.append(_line("chr5", 4294967295, "A", "ACC", ns))   # ten digits
    out.append(_line("chr5", 100, "A", "T", ns, ["0|0"] * ns))  # no sample carries it: no row
    return "".join(out).encode()


def near_misses(loci):
    """for every locus: one byte changed in each column, a prefix and an extension -- none of them a locus of the file"""
    have, out = set(loci), []
    for x in loci:
        c, p, r, a = x.split(b":")
        for y in ([c[:-1] + b"Z", p, r, a], [c, p[:-1] + (b"7" if p[-1:] != b"7" else b"8"), r, a], [c, p, b"N", a],
                  [c, p, r, a[:-1] + (b"N" if a[-1:] != b"N" else b"M")], [c, p + b"0", r, a], [c, p[:-1] or b"0", r, a], [c, p, r, a + a[-1:]],
                  [c, p, r, a[:-1] or b"+"], [c[3:] if c.startswith(b"chr") else b"chr" + c, p, r, a]):
            z = b":".join(y)
            if z not in have:
                out.append(z)
    return out


# loci of kinds_vcf that differ by a suffix, or are the ALTs of one line: the two lists of the file separate each pair
KIND_PAIRS = [(b"chr1:100:A:T", b"chr1:1000:A:T"), (b"chr3:2000:A:+AC", b"chr3:2000:A:+ACG"), (b"chr4:9001:C:-9", b"chr4:9001:C:-8"),
              (b"chr2:200:A:C", b"chr2:200:A:G"), (b"chr1:100:A:T", b"chr1:00100:A:T")]


def kinds_lists(loci):
    """two lists that are each other's complement over the file's loci, the first of every pair of KIND_PAIRS in the first:
    every locus is listed in one run and unlisted in the other"""
    distinct = sorted(set(loci))
    a = set(distinct[0::2])
    for x, y in KIND_PAIRS:
        a.add(x)
        a.discard(y)
    return sorted(a), sorted(set(distinct) - a)


def every_other(loci, first=0):
    """a selection that both keeps and drops: every second distinct locus"""
    return sorted(set(loci))[first::2]


@functools.lru_cache(maxsize=None)
def rows_vcf(n_rows, ns=3):
    """n_rows SNP rows, one per line, every one carried"""
    pat = ["0|1", "1|1", "1|0", "0|0", "./."]
    out = [vcfgen.header(ns)]
    for i in range(n_rows):
        gts = [pat[(i + 3 * s) % 5] for s in range(ns)]
        gts[i % ns] = "0|1"
        out.append(_line("chr%d" % (1 + i % 3), 1000 + i, "ACGT"[i % 4], "CGTA"[i % 4], ns, gts))
    return "".join(out).encode()


def rows_loci(n_rows):
    return [("chr%d:%d:%s:%s" % (1 + i % 3, 1000 + i, "ACGT"[i % 4], "CGTA"[i % 4])).encode() for i in range(n_rows)]


def third_of(n_rows):
    """the list of the run-shape cases: every third row, for n_rows == 1 the row itself"""
    return rows_loci(n_rows)[::3]


# ---- crafted tables: strings "chr1:<pos>:A:T" placed by the exported hash

def _hasher(bv):
    bv.lib.bvcf_locus_hash.restype = C.c_uint64
    bv.lib.bvcf_locus_hash.argtypes = [C.c_char_p, C.c_size_t]
    return bv.lib.bvcf_locus_hash


def snp_locus(pos):
    return b"chr1:%d:A:T" % pos


_PAIR = {}


def collision_pair(bv, capacity=16, limit=1 << 21):
    """the first two positions p < q whose loci agree in tag (h >> 32) and home slot at `capacity`: a birthday search over
    the strings chr1:<pos>:A:T -- 32 + log2(capacity) agreeing bits, about 2^20 strings for capacity 16"""
    if capacity not in _PAIR:
        h_of, seen = _hasher(bv), {}
        for pos in range(1, limit):
            s = snp_locus(pos)
            h = h_of(s, len(s))
            key = (h >> 32, h & (capacity - 1))
            if key in seen:
                _PAIR[capacity] = (seen[key], pos)
                break
            seen[key] = pos
        else:
            raise AssertionError("no pair below %d" % limit)
    return _PAIR[capacity]


def home_slot_positions(bv, slot, count, capacity=16, start=1):
    """the first `count` positions from `start` whose loci have home slot `slot` at `capacity`"""
    h_of, out, pos = _hasher(bv), [], start
    while len(out) < count:
        s = snp_locus(pos)
        if h_of(s, len(s)) & (capacity - 1) == slot:
            out.append(pos)
        pos += 1
    return out


def snps_vcf(positions, ns=2):
    """one carried SNP row chr1:<pos>:A:T per position"""
    return (vcfgen.header(ns) + "".join(_line("chr1", p, "A", "T", ns, ["0|1"] * ns) for p in positions)).encode()


def wrap_case(bv):
    """(listed positions, all positions of the file): four listed loci with home slot 15 of 16 -- the probe chain runs
    15, 0, 1, 2 --, and in the file also loci of home slots 15, 0 and 3 that are not listed, which walk the chain to its
    end"""
    listed = home_slot_positions(bv, 15, 4)
    others = (home_slot_positions(bv, 15, 2, start=listed[-1] + 1) + home_slot_positions(bv, 0, 2)
              + home_slot_positions(bv, 3, 2))
    return listed, sorted(set(listed + others))


def collision_case(bv):
    """(listed positions, positions of the file): the list holds A and C, the file B (A's partner in tag and home slot), C
    and D -- B and D go under keep, C goes under exclude"""
    a, b = collision_pair(bv)
    c, d = [p for p in range(1, 10) if p not in (a, b)][:2]
    return [a, c], sorted([b, c, d])


# ---- the file-level cases of tests/test_gpu_variant_list.py: name -> (vcf, loci of the list).  tests/test_variant_list_cpu.py
# checks, with the oracle alone, that every one both keeps and drops a row

def golden_list(oracle_body):
    return every_other(loci_of(oracle_body))


def pedigree_case():
    """the --mendel composition: (vcf, the .fam's bytes)"""
    import mendel
    import pairtable as pt
    vcf, trios = mendel.pedigree_vcf(30, 8, 120, 9310)
    return vcf, mendel.fam_of(trios, mendel.normalized(pt.sample_names(vcf)))


def round_trip_input():
    """(vcf, window) of the --ldPrune round trip: no locus twice, and the prune both keeps and drops"""
    import ldpairs
    return ldpairs.ld_vcf(9320, 40, 400), 50
