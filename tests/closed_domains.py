"""Closed input domains of the byte-parallel decoders, enumerated outright (pure Python, nothing read outside tests/).

The regular genotype scan (bvcf_gtscan.hip.h), the word-at-a-time getAlleles (eval_words / row_atoi9, bvcf_alleles.hip.h)
and the general field classifier (classify_field_g) decide on three bytes, two short strings and a number.  Those inputs
are few enough to list every one of them:

  G3   three-byte genotype fields a<sep>b: every byte next to 0 1 2 . and itself, and the whole square 0x20..0x3F
  GG   every string of length 0-4 over 0 1 2 . | / : and of length 5 over 0 1 . | / as a sample field
  R    REF x ALT token (and token pairs) over A C up to the lengths where the decisions change, padded to the word sizes,
       moved across the end of the staged head; POS shapes up to the ends of int64; CHROM over c h r 1

Every generator returns VCF bytes (header included) of one piece of a domain, cached; the tests hold each piece against the
oracle on every device chain (test_gpu_closed_domains.py) after test_closed_domains_cpu.py has shown, with the oracle alone,
that the pieces hold what they are meant to hold."""
import functools
import itertools
import re

import vcfgen

REFS = b"AGTC"  # REF of line i is REFS[i % 4]: each ALT of the lists below is valid (prints a row) next to one of them


def header(n_samples, eol=b"\n", with_format=True):
    return vcfgen.header(n_samples, with_format=with_format).encode().replace(b"\n", eol)


def gt_line(chrom, pos, ref, alt, fmt, fields, id_=b"."):
    return b"\t".join([chrom, pos, id_, ref, alt, b".", b"PASS", b".", fmt] + fields)


# ------------------------------------------------------------------ G3: three-byte genotype fields

G3_SAMPLES = 260
# 2 600 samples: more than the ten chunks of k_stream's line pipeline -- such lines are scanned one at a time, without the
# list mode.  2 500: the most chunks the pipeline takes, and a class-map slot (640 bytes) with room for the class lists of
# eight ALT indices (from 1 985 samples up)
G3_MANY_SAMPLES = (2600, 2500)
G3_ALT = b"G,T,C,GA,AT,ACC,TT,GG,CC"
G3_CARRIERS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 9))       # samples 0..4: every ALT index has a carrier
G3_MANY_CARRIERS = ((1, 2), (3, 4), (5, 6), (7, 8), (8, 8))  # ... of the eight that can have a class list
G3_DENSITIES = ("list", "dense")
G3_MANY_DENSITIES = ("list", "raw", "dense")
REGULAR_BYTES = frozenset(b"0123456789.")


@functools.lru_cache(maxsize=None)
def g3_probes():
    """a<sep>b and b<sep>a for a = every byte but TAB and LF, b one of 0 1 2 . a; plus the square a, b in 0x20..0x3F (the
    bytes the frame mask tor & 0xFFE0FFE0 lets through to the alphabet check) -> sorted tuple of 3-byte strings"""
    out = set()
    for sep in b"|/":
        for a in range(256):
            if a in (0x09, 0x0A):
                continue
            for b in (0x30, 0x31, 0x32, 0x2E, a):
                out.add(bytes((a, sep, b)))
                out.add(bytes((b, sep, a)))
        for a in range(0x20, 0x40):
            for b in range(0x20, 0x40):
                out.add(bytes((a, sep, b)))
    return tuple(sorted(out))


def is_regular(probe):
    """both sides a digit or a dot: what the regular scan classifies itself"""
    return len(probe) == 3 and probe[1] in b"|/" and probe[0] in REGULAR_BYTES and probe[2] in REGULAR_BYTES


@functools.lru_cache(maxsize=None)
def g3_square():
    """the probes of the 0x20..0x3F square: the 242 regular ones and every irregular one the frame mask lets through"""
    return tuple(p for p in g3_probes() if 0x20 <= p[0] < 0x40 and 0x20 <= p[2] < 0x40)


def g3_probe_at(i, ns=G3_SAMPLES, last=False):
    """the sample (0-based) that holds the probe of line i"""
    if last:
        return ns - 1
    return 8 + ((37 if ns == G3_SAMPLES else 373) * i) % (ns - 8)


def g3_fields(i, probe, ns, density, carriers, last=False):
    """the sample fields of line i: the reference genotype with the probe's separator, the carriers, the density's extra
    non-reference samples, the probe"""
    sep = probe[1:2]
    f = [b"0" + sep + b"0"] * ns
    if density == "dense":  # every third sample 0<sep>1: more non-reference lanes than a raw list holds
        het = b"0" + sep + b"1"
        for s in range(0, ns, 3):
            f[s] = het
    elif density == "dense2":  # ... 0<sep>1 and 0<sep>2 in turn: also more lanes with a digit >= 2 than a raw list holds
        for k, s in enumerate(range(0, ns, 3)):
            f[s] = b"0" + sep + (b"2" if k & 1 else b"1")
    elif density == "raw":  # 30 more lanes (4 samples each) with one non-reference sample: 16..63 lanes, all distinct
        for j in range(30):
            f[40 + 80 * j] = b"0" + sep + b"1"
    else:
        assert density == "list"
    for k, (x, y) in enumerate(carriers):
        f[k] = b"%d%s%d" % (x, sep, y)
    f[g3_probe_at(i, ns, last)] = probe
    return f


def g3_line(i, probe, ns=G3_SAMPLES, density="list", carriers=G3_CARRIERS, last=False):
    return gt_line(b"chr1", b"%d" % (1000 + i), REFS[i % 4:i % 4 + 1], G3_ALT, b"GT", g3_fields(i, probe, ns, density, carriers, last))


def _join(ns, lines, eol=b"\n"):
    return header(ns, eol) + eol.join(lines) + eol


@functools.lru_cache(maxsize=None)
def g3(density):
    """one line per probe at 260 samples, in list mode (carriers and probe only) or dense"""
    return _join(G3_SAMPLES, [g3_line(i, p, density=density) for i, p in enumerate(g3_probes())])


@functools.lru_cache(maxsize=None)
def g3_last(eol):
    """the square's probes as the last field, both densities, LF ("lf") or CRLF ("crlf") files: the terminator stands in
    for the TAB"""
    e = {"lf": b"\n", "crlf": b"\r\n"}[eol]
    both = [(d, p) for d in G3_DENSITIES for p in g3_square()]
    lines = [g3_line(i, p, density=d, last=True) for i, (d, p) in enumerate(both)]
    return _join(G3_SAMPLES, lines, e)


@functools.lru_cache(maxsize=None)
def g3_many(ns, density, regular_only=False):
    """the square's probes at 2 600 or 2 500 samples; density "list" (at most 15 map bytes), "raw" (16..63 non-reference
    lanes, all distinct) or "dense" """
    assert ns in G3_MANY_SAMPLES
    probes = [p for p in g3_square() if is_regular(p) or not regular_only]
    d = "dense2" if density == "dense" else density
    return _join(ns, [g3_line(i, p, ns, d, G3_MANY_CARRIERS) for i, p in enumerate(probes)])


@functools.lru_cache(maxsize=None)
def g3_regular(density):
    """the 242 regular probes alone at 260 samples (for the checks on the records of the streaming chain)"""
    probes = [p for p in g3_probes() if is_regular(p)]
    return _join(G3_SAMPLES, [g3_line(i, p, density=density) for i, p in enumerate(probes)])


# ------------------------------------------------------------------ GG: general genotype fields

GG_SAMPLES = 68
GG_ALT = b"G,T,C,GA,AT,ACC,TT,GG,CC,AG,TG"
GG_CARRIERS = (b"1/2", b"3/4", b"5/6", b"7/8", b"9/10", b"11/11")
GG_FORMS = ("gt", "gtdpgq")


@functools.lru_cache(maxsize=None)
def gg_probes():
    short = ["".join(t) for n in range(5) for t in itertools.product("012.|/:", repeat=n)]
    five = ["".join(t) for t in itertools.product("01.|/", repeat=5)]
    return tuple(s.encode() for s in short + five)


def gg_probe_at(i, last=False):
    return GG_SAMPLES - 1 if last else 8 + (37 * i) % (GG_SAMPLES - 8)


def gg_line(i, probe, form, last=False):
    tail = b":5:6" if form == "gtdpgq" else b""
    f = [b"0/0" + tail] * GG_SAMPLES
    for k, c in enumerate(GG_CARRIERS):
        f[k] = c + tail
    f[gg_probe_at(i, last)] = probe + tail
    return gt_line(b"chr2", b"%d" % (1000 + i), REFS[i % 4:i % 4 + 1], GG_ALT, b"GT:DP:GQ" if form == "gtdpgq" else b"GT", f)


@functools.lru_cache(maxsize=None)
def gg(form, last=False):
    """every probe once in a line of the form: bare under FORMAT GT, or with :5:6 appended under GT:DP:GQ"""
    return _join(GG_SAMPLES, [gg_line(i, p, form, last) for i, p in enumerate(gg_probes())])


# ------------------------------------------------------------------ R: REF, ALT, POS and CHROM

R_SAMPLES = 3
R_LONG_SAMPLES = 70  # lines of more than 256 + 3 bytes: k_stream hands k_order a TAB bitmap of the head only for such lines
R_FIELDS = [b"0/1", b"1/2", b"2/2"]  # genotypes that carry both tokens of a pair
POS9 = b"123456789"
# kHeadRowBytes: the bytes of a line k_head stages.  A hand copy of BVCF_HEAD_STAGE (csrc/bvcf_head.hip.h), which the library
# does not export: it has to follow that constant, or the row-edge block no longer straddles the end of the staged head
HEAD_ROW_BYTES = 64


def _over(alphabet, lo, hi):
    return [("".join(t)).encode() for n in range(lo, hi + 1) for t in itertools.product(alphabet, repeat=n)]


R_REFS = _over("AC", 1, 4) + [b"N", b"AN", b"NA", b""]
R_TOKENS = _over("AC", 1, 5) + [b"N", b"AN", b"NA", b"", b"*", b"a", b"."]
R_FIRST_TOKENS = [b"A", b"C", b"AC", b"CA", b"ACA", b"N", b""]
R_EDGE_TOTALS = (7, 8, 9, 15, 16, 17)  # around the 8- and 16-byte words of eval_words


def r_single():
    return [(ref, tok) for ref in R_REFS for tok in R_TOKENS]


def r_pairs():
    return [(ref, t1 + b"," + t2) for ref in _over("AC", 1, 3) for t1 in R_FIRST_TOKENS for t2 in R_TOKENS]


def r_wordsize():
    """REF and token padded with the same run of G, on the left (a common prefix) or on the right (a common suffix), so
    that the longer of the two has the total length"""
    out = []
    for ref in _over("AC", 1, 3):
        for tok in _over("AC", 1, 4):
            for total in R_EDGE_TOTALS:
                pad = b"G" * (total - max(len(ref), len(tok)))
                out.append((pad + ref, pad + tok))
                out.append((ref + pad, tok + pad))
    return out


def r_first_three():
    return r_single() + r_pairs() + r_wordsize()


def r_rowedge():
    """a 300-line subset with ID lengths that put REF's first byte at every offset from 24 bytes before the end of the
    staged head to 2 bytes past it -> [(pos, id, ref, alt)]"""
    subset = r_first_three()[::47][:300]
    assert len(subset) == 300
    out = []
    for off in range(HEAD_ROW_BYTES - 24, HEAD_ROW_BYTES + 3):
        for i, (ref, alt) in enumerate(subset):
            pos = POS9[:i % 9 + 1]
            out.append((pos, b"i" * (off - len(pos) - 4), ref, alt))  # CHROM "1": REF starts at 1 + 1 + len(pos) + 1 + len(id) + 1
    return out


R_POS = [b"0", b"1", b"7", b"+7", b"-7", b"+0", b"-0", b"007",
         b"", b"+", b"-", b"1e3", b"1.0", b" 7", b"7 ", b"0x10", b"1_000",
         b"123456789", b"999999999", b"1000000000", b"1234567890",
         b"9223372036854775806", b"9223372036854775807", b"9223372036854775808",
         b"-9223372036854775808", b"-9223372036854775809", b"+9223372036854775807",
         b"99999999999999999999", b"00000000000000000000123", "١٢٣".encode()]  # (the last one: Arabic-Indic digits)
R_POS_PAIRS = [(b"A", b"C"), (b"AC", b"A"), (b"AC", b"A,C"), (b"A", b"AC"), (b"AC", b"ACC"), (b"ACC", b"AC"), (b"AC", b"CA"),
               (b"ACG", b"A,AT"), (b"AC", b"C"), (b"AC", b"N")]
# POS + 1 or POS + offset leaves int64 from these: Go's addition wraps, and the row prints -9223372036854775808
R_POS_WRAPS = (b"9223372036854775807", b"+9223372036854775807")
R_POS_WRAP_PAIRS = ((b"AC", b"A"), (b"AC", b"A,C"), (b"ACC", b"AC"), (b"AC", b"CA"), (b"ACG", b"A,AT"))


def r_pos_chrom(k, j):
    """the CHROM of POS shape k with REF/ALT pair j: it names the line in the output"""
    return b"chr%d" % (10 * k + j)


R_BLOCKS = ("single", "pairs", "wordsize", "rowedge", "pos", "chrom")


def r_records(block):
    """-> [(chrom, pos, id, ref, alt)] of one block"""
    if block in ("single", "pairs", "wordsize"):
        pairs = {"single": r_single, "pairs": r_pairs, "wordsize": r_wordsize}[block]()
        return [(b"1", POS9[:i % 9 + 1], b".", ref, alt) for i, (ref, alt) in enumerate(pairs)]
    if block == "rowedge":
        return [(b"1", pos, id_, ref, alt) for pos, id_, ref, alt in r_rowedge()]
    if block == "pos":
        return [(r_pos_chrom(k, j), pos, b".", ref, alt) for k, pos in enumerate(R_POS) for j, (ref, alt) in enumerate(R_POS_PAIRS)]
    if block == "chrom":
        return [(c, b"100", b".", b"A", b"C") for c in _over("chr1", 0, 5)]
    raise KeyError(block)


@functools.lru_cache(maxsize=None)
def r(block, samples=R_SAMPLES):
    """one block with three samples (or 70: the three and the reference genotype), or as a sites-only file (samples = 0: no
    FORMAT and sample columns)"""
    tail = [b"GT"] + R_FIELDS + [b"0/0"] * (samples - len(R_FIELDS)) if samples else []
    lines = [b"\t".join([chrom, pos, id_, ref, alt, b".", b"PASS", b"."] + tail) for chrom, pos, id_, ref, alt in r_records(block)]
    return header(samples, with_format=samples > 0) + b"\n".join(lines) + b"\n"


# ------------------------------------------------------------------ the pieces by name

def lines_part(vcf, k, n):
    """the header and the k-th of n equal runs of the data lines of `vcf` (each line as it is in the whole file)"""
    head, lines = vcf.split(b"\n")[:3], vcf.split(b"\n")[3:-1]
    per = (len(lines) + n - 1) // n
    return b"\n".join(head + lines[k * per:(k + 1) * per]) + b"\n"


@functools.lru_cache(maxsize=64)
def piece(name):
    """"g3-list", "g3_last-crlf", "g3_2600-raw", "gg-gtdpgq", "gg-gt-last", "r-pairs", "r-pairs-sites", "r-pairs-long" -> the
    VCF bytes; with "-part2of4" behind the name the third quarter of the piece's lines"""
    part = re.search(r"-part(\d+)of(\d+)$", name)
    if part:
        return lines_part(piece(name[:part.start()]), int(part.group(1)), int(part.group(2)))
    kind, *args = name.split("-")
    if kind == "gg":
        return gg(args[0], args[1:] == ["last"])
    if kind == "r":
        return r(args[0], {"sites": 0, "long": R_LONG_SAMPLES}[args[1]] if args[1:] else R_SAMPLES)
    if kind in ("g3_2600", "g3_2500"):
        return g3_many(int(kind[3:]), *args)
    return {"g3": g3, "g3_last": g3_last}[kind](*args)
