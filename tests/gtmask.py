"""--minGQ / --minDP: the masking rules of include/bvcf.h applied to VCF text, and the inputs the tests of the flag share.

The oracle knows nothing of the flag.  What a masked run must produce follows from an equivalence instead:

    device run of the ORIGINAL bytes with the thresholds  ==  oracle run of mask_vcf(bytes) without them

mask_vcf replaces the genotype subfield of every masked sample field with "./." and touches nothing else."""
import collections
import functools
import random

import vcfgen

DIGITS = frozenset(b"0123456789")
MAX_THRESHOLD = 999999999


def key_index(fmt, key):
    """rule 1: the first position >= 1 of the FORMAT column whose text is exactly `key`, or None"""
    keys = fmt.split(b":")
    for k in range(1, len(keys)):
        if keys[k] == key:
            return k
    return None


def is_number(value):
    """rule 2: 1 to 9 bytes, all ASCII digits"""
    return value is not None and 1 <= len(value) <= 9 and all(ch in DIGITS for ch in value)


def field_masked(field, k, threshold):
    """rules 2-3 for one sample field and one key: (has a number, the number is below the threshold)"""
    if k is None or threshold <= 0:
        return False, False
    sub = field.split(b":")
    value = sub[k] if k < len(sub) else None
    if not is_number(value):
        return False, False
    return True, int(value) < threshold


def mask_line(line, min_gq, min_dp, stats=None):
    """one data line without its terminator -> the line with the genotype of every masked sample field set to ./."""
    cols = line.split(b"\t")
    if len(cols) <= 9:
        return line
    kq = key_index(cols[8], b"GQ") if min_gq > 0 else None
    kd = key_index(cols[8], b"DP") if min_dp > 0 else None
    if kq is None and kd is None:
        return line
    for i in range(9, len(cols)):
        has_q, low_q = field_masked(cols[i], kq, min_gq)
        has_d, low_d = field_masked(cols[i], kd, min_dp)
        if stats is not None and (has_q or has_d):
            stats["valued"] += 1
        if low_q or low_d:  # rule 4: either key masks
            if stats is not None:
                stats["masked"] += 1
            sub = cols[i].split(b":")
            sub[0] = b"./."
            cols[i] = b":".join(sub)
    return b"\t".join(cols)


def mask_vcf(vcf_bytes, min_gq=0, min_dp=0, stats=None):
    """rules 1-5 applied literally to the text; CRLF is kept.  stats (optional dict): "valued" counts the sample fields
    in which an active key has a number, "masked" those whose genotype was replaced"""
    assert 0 <= min_gq <= MAX_THRESHOLD and 0 <= min_dp <= MAX_THRESHOLD
    if stats is not None:
        stats.setdefault("valued", 0)
        stats.setdefault("masked", 0)
    lines = vcf_bytes.split(b"\n")
    crlf = len(lines) > 1 and lines[0].endswith(b"\r")
    seen_header = False
    for i, ln in enumerate(lines):
        if not seen_header:
            seen_header = ln.startswith(b"#CHROM")
            continue
        cr = b"\r" if crlf and ln.endswith(b"\r") else b""
        body = ln[:len(ln) - len(cr)]
        lines[i] = mask_line(body, min_gq, min_dp, stats) + cr
    return b"\n".join(lines)


# ---- crafted FORMAT shapes (vcfgen.py is shared and only knows GT and GT:DP:GQ)

FORMATS = ["GT:AD:DP:GQ:PL", "GT:AD:DP:GQ:PL", "GT:GQ:DP", "GT:DP:GQ", "GT", "GT:DP", "GT:GQ", "GT:AD:PL", "GQ:GT:DP",
           "GT:GQX:DP", "GT:GQ:GQ:DP", "GT:DPX:XDP:GQ", "GT:PL:GQ", "GT:AD:DP:GQ:PL:GQ"]
ODD_VALUES = [".", "", "007", "12.5", "-3", "1e2", "123456789", "1234567890", "0", "19", "20", "9", "10", "+5", "000000005",
              "0000000005", "99999999999", "5 ", "٣"]
CALLS = ["0/0"] * 12 + ["0/1", "0/1", "1/1", "1|0", "0|1", "./.", ".|.", "1", "0", ".", "0/1/1", "1/1/1", "0/0/0", "0/."]


def pl_list(rng, n):
    return ",".join(str(rng.randint(0, 999)) for _ in range(n))


def crafted_vcf(seed, ns=37, n_lines=180, eol="\n"):
    """lines of many FORMAT shapes: keys at any index, missing, repeated or merely similar; odd values; trailing subfields
    dropped; long PL lists in front of GQ (fields past 64 and past 1 024 bytes); haploid and polyploid calls; multiallelic
    lines of 2-9 ALTs and MNPs; lines that a single sample carries (masked, their row disappears)"""
    rng = random.Random(seed)
    out = [vcfgen.header(ns)]
    pos = 5000
    for li in range(n_lines):
        pos += rng.randint(1, 90)
        kind = rng.random()
        if kind < 0.12:
            ref, alts = "ACG", ["TCA"]  # MNP
        elif kind < 0.37:
            n_alt = rng.randint(2, 9)
            ref = "A"
            alts = [rng.choice(["C", "G", "T", "AT", "ACC", "AG"]) for _ in range(n_alt)]
            alts = list(dict.fromkeys(alts)) if rng.random() < 0.5 else alts
        else:
            ref = rng.choice("ACGT")
            alts = [rng.choice([b for b in "ACGT" if b != ref])]
        n_alt = len(alts)
        fmt = FORMATS[li % len(FORMATS)] if li < 3 * len(FORMATS) else rng.choice(FORMATS)
        keys = fmt.split(":")
        single = rng.random() < 0.25  # one carrier only
        carrier = rng.randrange(ns)
        fields = []
        for s in range(ns):
            if single:
                call = "0/1" if s == carrier else "0/0"
            elif n_alt > 1 and rng.random() < 0.4:
                call = "%d%s%d" % (rng.randint(0, n_alt), rng.choice("|/"), rng.randint(0, n_alt))
            else:
                call = rng.choice(CALLS)
            sub = []
            for key in keys:
                if key == "GT":
                    sub.append(call)
                elif key == "AD":
                    sub.append(",".join(str(rng.randint(0, 40)) for _ in range(n_alt + 1)))
                elif key == "PL":
                    r = rng.random()
                    n_pl = 400 if r < 0.004 else (30 if r < 0.04 else 3)  # > 1 024 bytes, > 64 bytes, the usual
                    sub.append(pl_list(rng, n_pl))
                else:
                    sub.append(rng.choice(ODD_VALUES) if rng.random() < 0.2 else str(rng.randint(0, 99)))
            if rng.random() < 0.1:
                sub = sub[:rng.randint(1, len(sub))]  # trailing subfields dropped
            fields.append(":".join(sub))
        cols = ["chr2", str(pos), ".", ref, ",".join(alts), "50", "PASS", "DP=9", fmt] + fields
        out.append("\t".join(cols) + "\n")
    s = "".join(out)
    return (s.replace("\n", eol) if eol != "\n" else s).encode()


def alignment_vcf(eol="\n"):
    """the value of a masked field at every byte alignment: the first sample's AD subfield grows a byte a line, over the 16
    bytes of a lane and across the first 1 KiB chunk boundary of the sample region; the samples behind it alternate
    between GQ 5 (masked by --minGQ 20) and GQ 50"""
    ns = 12
    out = [vcfgen.header(ns)]
    pos = 100
    for li, pad in enumerate(list(range(1, 50)) + list(range(960, 1060))):
        pos += 7
        kept_call = "0/0" if li % 10 == 9 else "0/1"  # every tenth line: only masked samples carry, the row disappears
        fields = ["%s:%s:30:50" % (kept_call, "1" * pad)]
        for s in range(1, ns):
            if s % 2:
                fields.append("0/1:3,4:30:5" if s != ns - 1 else "1/1:3,4:2:5")
            else:
                fields.append("%s:3,4:30:50" % kept_call)
        out.append("\t".join(["chr3", str(pos), ".", "G", "T", "50", "PASS", "DP=9", "GT:AD:DP:GQ"] + fields) + "\n")
    s = "".join(out)
    return (s.replace("\n", eol) if eol != "\n" else s).encode()


def wide_vcf(seed=91, ns=33000, n_lines=5):
    """a few lines of a cohort past BVCF_WIDE_SAMPLES samples, GT:DP:GQ"""
    rng = random.Random(seed)
    out = [vcfgen.header(ns)]
    for li in range(n_lines):
        fields = []
        for s in range(ns):
            r = rng.random()
            call = "0/0" if r < 0.9 else rng.choice(["0/1", "1/1", "./.", "1|0"])
            if li == n_lines - 1:
                call = "0/1" if s == 4321 else "0/0"  # one carrier, DP 3 and GQ 3: the row disappears under either threshold
                fields.append("%s:%d:%d" % ((call, 3, 3) if s == 4321 else (call, rng.randint(0, 99), rng.randint(0, 99))))
            else:
                fields.append("%s:%d:%d" % (call, rng.randint(0, 99), rng.randint(0, 99)))
        out.append("\t".join(["chr4", str(1000 + 10 * li), ".", "C", "T", "50", "PASS", "DP=9", "GT:DP:GQ"] + fields) + "\n")
    return "".join(out).encode()


def rare_tail(vcf, seed):
    """a vcfgen GT:DP:GQ file with eight lines behind it that one sample carries: with a cohort's worth of carriers per
    line no mask ever empties a row of vcfgen's own; the carrier's (DP, GQ) goes through low / high pairs, so some of
    these rows disappear under either threshold and the others stay"""
    rng = random.Random(seed)
    lines = vcf.split(b"\n")
    eol = "\r\n" if lines[0].endswith(b"\r") else "\n"
    ns = next(ln for ln in lines if ln.startswith(b"#CHROM")).rstrip(b"\r").count(b"\t") - 8
    out = []
    for i, (dp, gq) in enumerate([(5, 50), (50, 5), (3, 3), (50, 50)] * 2):
        carrier = rng.randrange(ns)
        fields = ["%s:%d:%d" % (("0/1", dp, gq) if s == carrier else ("0|0", rng.randint(0, 99), rng.randint(0, 99)))
                  for s in range(ns)]
        out.append("\t".join(["chr9", str(900000 + 10 * i), ".", "A", "G", "50", "PASS", "DP=9", "GT:DP:GQ"] + fields) + eol)
    return vcf + "".join(out).encode()


# ---- the seeded inputs of tests/test_gpu_gt_filter.py: name -> (maker of the VCF bytes, oracle config)
# (test_gt_filter_cpu.py checks, with the oracle alone, that the mask bites on every one of them under every threshold pair)

THRESHOLDS = [(20, 0), (0, 10), (20, 10)]  # (minGQ, minDP): GQ only, DP only, both

FUZZ = {
    "fuzz17": (lambda: rare_tail(vcfgen.gen_vcf(61, 320, 17, True, weird=0.08), 1), {"allow": ""}),
    "fuzz70crlf": (lambda: rare_tail(vcfgen.gen_vcf(62, 260, 70, True, weird=0.05, eol="\r\n"), 2), {}),
    "fuzz300": (lambda: rare_tail(vcfgen.gen_vcf(63, 200, 300, True, weird=0.03), 3),
                {"keepId": True, "keepInfo": True, "keepPos": True, "fieldDelimiter": ",", "emptyField": "NA"}),
    "fuzz2600crlf": (lambda: rare_tail(vcfgen.gen_vcf(64, 70, 2600, True, weird=0.02, eol="\r\n"), 4), {"allow": ""}),
}
CRAFTED = {
    "crafted37": (lambda: crafted_vcf(71), {}),
    "crafted5crlf": (lambda: crafted_vcf(72, ns=5, n_lines=260, eol="\r\n"), {}),
    "crafted130": (lambda: crafted_vcf(73, ns=130, n_lines=120), {"keepInfo": True}),
    "alignment": (alignment_vcf, {}),
    "alignment_crlf": (lambda: alignment_vcf("\r\n"), {}),
}
OTHER = {
    "wide33000": (wide_vcf, {}),
    "cohort": (lambda: rare_tail(vcfgen.gen_vcf(81, 2500, 400, True, weird=0.02) +
                                 vcfgen.gen_vcf(82, 1200, 400, True, weird=0.02).split(b"\n", 3)[3], 5), {}),
    "stats300": (lambda: rare_tail(vcfgen.gen_vcf(83, 300, 300, True, weird=0.04), 6), {}),
}
SEEDED = dict(FUZZ, **CRAFTED, **OTHER)


@functools.lru_cache(maxsize=None)
def seeded(name):
    return SEEDED[name][0]()


@functools.lru_cache(maxsize=None)
def masked(name, min_gq, min_dp):
    """(masked bytes, stats) of a seeded input"""
    st = {}
    return mask_vcf(seeded(name), min_gq, min_dp, st), st


def thresholds_of(name):
    """the alignment files only carry GQ values worth masking"""
    return [(20, 0), (20, 10)] if name.startswith("alignment") else THRESHOLDS


def row_changes(body_orig, body_masked, header_cols):
    """(rows that disappeared, rows that kept their place with another heterozygotes / missingGenos list), by the first
    five columns of the TSV (chrom, pos, type, ref, alt)"""
    ih, im = header_cols.index("heterozygotes"), header_cols.index("missingGenos")

    def rows(body):
        d = collections.OrderedDict()
        for r in body.split(b"\n"):
            if r:
                f = r.split(b"\t")
                d.setdefault(tuple(f[:5]), []).append((f[ih], f[im]))
        return d
    a, b = rows(body_orig), rows(body_masked)
    gone = [k for k in a if k not in b]
    changed = [k for k in a if k in b and a[k] != b[k]]
    return gone, changed
