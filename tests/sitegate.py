"""--minMaf / --maxMaf / --minMac / --maxMissing / --hwe: the expected verdicts, written from the definitions in
include/bvcf.h (bvcf_set_site_gate), not from the kernel.

A row of the TSV carries everything the gate looks at: ac, an and the three sample lists.  gate() decides every row of an
oracle run; the expected TSV is the oracle's with the failing rows taken out, the expected --sampleStats / --relatedness
tables are the ones of the rows that stay.  Test infrastructure only."""
import functools
import random
from fractions import Fraction

import vcfgen
from pairtable import BASE_HEADER, snp_line

REPORT = ["examined", "kept", "minMaf", "maxMaf", "minMac", "maxMissing", "hwe"]
BITS = {"minMaf": 1, "maxMaf": 2, "minMac": 4, "maxMissing": 8, "hwe": 16}
NEUTRAL = {"minMaf": 0.0, "maxMaf": 1.0, "minMac": 0, "maxMissing": 1.0, "hwe": 0.0}
TIE = (10 ** 7 + 1, 10 ** 7)  # 1 + 1e-7 as a ratio of integers
HWE_TOL = 1e-9      # device and reference p values: relative, or ...
HWE_TINY = 1e-280   # ... both below this


@functools.lru_cache(maxsize=None)
def _factorials(n):
    f = [1] * (n + 1)
    for i in range(2, n + 1):
        f[i] = f[i - 1] * i
    return f


def support(a, b, c):
    """(n, r, the het counts h of the support) of the exact test on a het, b hom, c other called samples"""
    n = a + b + c
    r = a + 2 * min(b, c)
    return n, r, range(r & 1, r + 1, 2)


def weights_exact(a, b, c):
    """w(h) = n! 2^h / (((r-h)/2)! h! (n - h - (r-h)/2)!) over the support, as Python integers: the first from the
    factorials, the others by w(h+2) = w(h) 4 hr hc / ((h+2)(h+1)), an exact division"""
    n, r, hs = support(a, b, c)
    f = _factorials(n)
    h = hs[0]
    hr = (r - h) // 2
    w = f[n] * (1 << h) // (f[hr] * f[h] * f[n - h - hr])
    out = [w]
    for h in hs[:-1]:
        hr = (r - h) // 2
        num, den = w * 4 * hr * (n - h - hr), (h + 2) * (h + 1)
        assert num % den == 0
        w = num // den
        out.append(w)
    return out


def hwe_exact_rational(a, b, c):
    """p_hwe as a Fraction: sum of the w(h) <= w(a) (1 + 1e-7) over the sum of all, in exact arithmetic"""
    w = weights_exact(a, b, c)
    wa = w[a // 2]
    tail = sum(x for x in w if x * TIE[1] <= wa * TIE[0])
    return Fraction(tail, sum(w))


def tie_margin(a, b, c):
    """the smallest |w(h) / w(a) - (1 + 1e-7)| over the support, ratios that equal 1 left out (a Fraction, or None)"""
    w = weights_exact(a, b, c)
    wa = w[a // 2]
    lim = Fraction(*TIE)
    d = [abs(Fraction(x, wa) - lim) for x in w if x != wa]
    return min(d) if d else None


def near_tie(a, b, c):
    """is some w(h) / w(a), other than a ratio of exactly 1, within 1e-9 of 1 + 1e-7?  (tie_margin(...) <= 1e-9, by
    cross-multiplied integers: 1 + 1e-7 -+ 1e-9 = 1 000 000 099 / 1e9 and 1 000 000 101 / 1e9)"""
    w = weights_exact(a, b, c)
    wa = w[a // 2]
    lo, hi = wa * 1000000099, wa * 1000000101
    return any(x != wa and lo <= x * 10 ** 9 <= hi for x in w)


def hwe_p(a, b, c):
    """p_hwe in float64: every term relative to the largest, by the recurrence w(h+2) / w(h) = 4 hr hc / ((h+2)(h+1))
    outwards from it"""
    n, r, hs = support(a, b, c)
    k = len(hs)
    if k == 1:
        return 1.0
    par = r & 1

    def up(i):  # w(index i + 1) / w(index i)
        h = par + 2 * i
        hr = r // 2 - i
        return (4.0 * hr * (n - h - hr)) / ((h + 2.0) * (h + 1.0))

    m = min(k - 1, max(0, int(r * (2 * n - r) / (2.0 * n)) // 2))
    while m + 1 < k and up(m) > 1.0:
        m += 1
    while m > 0 and up(m - 1) < 1.0:
        m -= 1
    t = [0.0] * k
    t[m] = 1.0
    for i in range(m, k - 1):
        t[i + 1] = t[i] * up(i)
    for i in range(m, 0, -1):
        t[i - 1] = t[i] / up(i - 1)
    thr = t[a // 2] * (1.0 + 1e-7)
    return min(1.0, sum(x for x in t if x <= thr) / sum(t))


@functools.lru_cache(maxsize=None)
def hwe_ref(a, b, c):
    """the yardstick: the rational value up to n = 3 000, hwe_p (tied to it below that by the CPU tests) above"""
    return float(hwe_exact_rational(a, b, c)) if a + b + c <= 3000 else hwe_p(a, b, c)


def close(got, want):
    """the tolerance for p values compared as numbers"""
    if got != got or want != want:
        return False
    return abs(got - want) <= HWE_TOL * abs(want) or (abs(got) < HWE_TINY and abs(want) < HWE_TINY)


def row_counts(fields, cfg=None, header=BASE_HEADER):
    """(ac, an, n_het, n_hom, n_miss) of a TSV row split at TABs"""
    cfg = cfg or {}
    delim, empty = cfg.get("fieldDelimiter", ";").encode(), cfg.get("emptyField", "!").encode()
    n = [0 if fields[header.index(x)] == empty else fields[header.index(x)].count(delim) + 1
         for x in ("heterozygotes", "homozygotes", "missingGenos")]
    return int(fields[header.index("ac")]), int(fields[header.index("an")]), n[0], n[1], n[2]


def triple(S, n_het, n_hom, n_miss):
    n = S - n_miss
    return n_het, n_hom, n - n_het - n_hom


def verdict(criteria, S, counts, p_of=hwe_ref):
    """the fail bits of an examined row"""
    cr = dict(NEUTRAL, **criteria)
    ac, an, n_het, n_hom, n_miss = counts
    mac = min(ac, an - ac)
    bits = 0
    if float(mac) / float(an) < cr["minMaf"]:
        bits |= BITS["minMaf"]
    if float(mac) / float(an) > cr["maxMaf"]:
        bits |= BITS["maxMaf"]
    if mac < cr["minMac"]:
        bits |= BITS["minMac"]
    if float(n_miss) / float(S) > cr["maxMissing"]:
        bits |= BITS["maxMissing"]
    if cr["hwe"] > 0 and p_of(*triple(S, n_het, n_hom, n_miss)) < cr["hwe"]:
        bits |= BITS["hwe"]
    return bits


def gate(tsv_body, S, criteria, cfg=None, header=BASE_HEADER):
    """-> (mask: True for the rows that stay, the seven counts of the report, the report's text) of a TSV body (no header
    line); every row of a file with samples is an examined row"""
    rows = [r for r in tsv_body.split(b"\n") if r]
    counts = [0] * 7
    mask = []
    for r in rows:
        bits = verdict(criteria, S, row_counts(r.split(b"\t"), cfg, header)) if S else 0
        mask.append(bits == 0)
        if S:
            counts[0] += 1
            counts[1] += bits == 0
            for q in range(5):
                counts[2 + q] += (bits >> q) & 1
    return mask, counts, report_text(counts)


def report_text(counts):
    return "".join("%s\t%d\n" % (nm, v) for nm, v in zip(REPORT, counts)).encode()


def kept_body(tsv_body, mask):
    rows = [r for r in tsv_body.split(b"\n") if r]
    return b"".join(r + b"\n" for r, k in zip(rows, mask) if k)


def row_p_values(tsv_body, S, cfg=None, header=BASE_HEADER):
    """the reference p_hwe of every row"""
    return [hwe_ref(*triple(S, *row_counts(r.split(b"\t"), cfg, header)[2:])) for r in tsv_body.split(b"\n") if r]


def cli_args(criteria, report=None):
    a = []
    for k, v in criteria.items():
        a += ["--" + k, repr(v) if isinstance(v, float) else str(v)]
    return a + (["--siteFilterReport", str(report)] if report else [])


# ---- inputs

def hwe_sweep_vcf(ns=300, seed=9100):
    """rows swept from an excess of homozygotes through Hardy-Weinberg equilibrium to an excess of heterozygotes, at
    allele frequencies from rare to 0.5: biallelic rows, multiallelic rows (each ALT against the rest) and rows with
    missing calls.  (The seeded inputs of pairtable.py draw both alleles of a call independently: they sit in
    equilibrium by construction.)"""
    rng = random.Random(seed)
    out = [vcfgen.header(ns)]
    pos = 1000
    for q in (0.01, 0.03, 0.1, 0.25, 0.4, 0.5):
        for f in (-0.9, -0.5, -0.25, -0.1, 0.0, 0.1, 0.25, 0.5, 0.9):  # inbreeding coefficient: het = 2pq (1 - f)
            for miss in (0.0, 0.03, 0.3):
                pos += 10
                p_het = max(0.0, min(1.0, 2 * q * (1 - q) * (1 - f)))
                p_hom = max(0.0, q * q + q * (1 - q) * f)
                gts = []
                for _ in range(ns):
                    u = rng.random()
                    if rng.random() < miss:
                        gts.append(rng.choice(["./.", ".|."]))
                    elif u < p_het:
                        gts.append(rng.choice(["0|1", "1|0", "0/1"]))
                    elif u < p_het + p_hom:
                        gts.append("1|1")
                    else:
                        gts.append("0|0")
                gts[rng.randrange(ns)] = "0|1"
                out.append(snp_line(pos, gts))
    for q in (0.05, 0.2, 0.35):  # two ALTs: each emitted row is "this ALT against the rest"
        for f in (-0.6, 0.0, 0.6):
            pos += 10
            gts = []
            for _ in range(ns):
                if rng.random() < 0.02:
                    gts.append("./.")
                    continue
                x = rng.choices([0, 1, 2], [1 - 2 * q, q, q])[0]
                y = x if rng.random() < max(f, 0.0) else rng.choices([0, 1, 2], [1 - 2 * q, q, q])[0]
                if f < 0 and x == y and rng.random() < -f:
                    y = (x + 1) % 3
                gts.append("%d|%d" % (x, y))
            out.append("\t".join(["chr3", str(pos), ".", "A", "C,G", "50", "PASS", ".", "GT"] + gts) + "\n")
    return "".join(out).encode()


def seeded_triples(n, count, seed):
    """(het, hom, other) with het + hom + other = n: around equilibrium at a random allele frequency, pushed towards an
    excess of either kind; plus the corners"""
    rng = random.Random(seed * 1000003 + n)
    out = [(n, 0, 0), (0, n // 2, n - n // 2), (0, 0, n), (min(n, 1), 0, n - min(n, 1))]
    while len(out) < count + 4:
        q = rng.choice([rng.random() * 0.5, rng.random() ** 3 * 0.5])
        f = rng.choice([0.0, rng.uniform(-1, 1), rng.uniform(-0.1, 0.1)])
        het = int(round(n * 2 * q * (1 - q) * (1 - f)))
        hom = int(round(n * (q * q + q * (1 - q) * f)))
        het = max(0, min(n, het + rng.randint(-2, 2)))
        hom = max(0, min(n - het, hom + rng.randint(-1, 1)))
        out.append((het, hom, n - het - hom))
    return out


# ---- the triples the device's exact test is run on (bvcf_bench_hwe): shared by tests/test_gpu_site_gate.py, which runs
# them, and tests/test_site_gate_cpu.py, which checks their term ratios against the tie factor

DEVICE_SIZES = [63, 64, 65, 2504, 10000, 100000]
ALL_HET = [(n, 0, 0) for n in (1, 2, 63, 64, 65, 127, 128, 129, 200, 1000)]
ONE_TERM = [(0, 0, 1), (0, 0, 64), (0, 100000, 0), (0, 0, 100000), (1, 0, 99999), (0, 0, 0)]  # p = 1
UNDERFLOW = (0, 50000, 50000)  # 25 001 terms, the observed one 1e-30000 of the mode
# every lane's segment and the wave's partial last segment: supports of 64 k + j terms
SEGMENTS = [(2 * (k - 1), 0, 4000) for k in (33, 63, 64, 65, 127, 128, 129, 640, 641, 1253)]
MARGIN_CHECK_MAX_N = 10000  # the tie-factor condition is checked in exact integers up to here (weights of 100 000 calls are too long)


def device_triples(n):
    """the seeded triples of one size and, where n allows them, supports of 31 .. 34 terms: both sides of the inline / wave
    bound (32 terms) and the bound itself"""
    tr = seeded_triples(n, 24, 2)
    return tr + [(r - 2 * k, k, n - r + k) for r in (61, 62, 63, 64, 65, 66) for k in (0, 1, 5) if r <= n and n - r + k >= k]


def all_device_triples():
    out = set(small_triples(12)) | set(ALL_HET) | set(ONE_TERM) | set(SEGMENTS) | {UNDERFLOW}
    for n in DEVICE_SIZES:
        out.update(device_triples(n))
    return sorted(out)


def small_triples(n_max=12):
    """every (het, hom, other) with n <= n_max"""
    return [(a, b, n - a - b) for n in range(n_max + 1) for a in range(n + 1) for b in range(n - a + 1)]


# ---- the file-level cases: input name -> the criteria sets it is run with.  tests/test_site_gate_cpu.py checks, with the
# oracle alone, that every set both keeps and drops a row under each of its criteria (inputs of one row and of one
# sample, which cannot do both at once, come with sets that keep and sets that drop), that no row's p value lies within
# 1e-6 of a tested --hwe value, and that no term ratio of a row lies within 1e-9 of the tie factor.

RARE = {"minMaf": 0.02, "maxMaf": 0.1, "minMac": 3, "maxMissing": 0.03, "hwe": 0.01}
WIDE = {"minMaf": 0.004, "maxMaf": 0.1, "minMac": 2, "maxMissing": 0.045, "hwe": 1e-7}  # (leaves the 300-sample files more rows)
TILE = {"minMaf": 0.4, "maxMaf": 0.45, "minMac": 47, "maxMissing": 0.15, "hwe": 0.1}
TILE_DROPS = {"minMaf": 0.45, "maxMaf": 0.4, "minMac": 60, "maxMissing": 0.1, "hwe": 0.5}  # fails the single row of tile_vcf(1) five times
SWEEP = {"minMaf": 0.05, "maxMaf": 0.45, "minMac": 10, "maxMissing": 0.1, "hwe": 1e-6}
FUZZ13 = {"minMaf": 0.05, "maxMaf": 0.15, "minMac": 20, "maxMissing": 0.12, "hwe": 1e-10}
MASKED13 = dict(FUZZ13, maxMissing=0.3)  # (--minGQ 20 makes a fifth to a third of every row's calls missing)
GOLDEN = {"minMaf": 0.01, "maxMaf": 0.3, "minMac": 5, "hwe": 1e-6}  # (the slice has no missing call)
ONE_SAMPLE = {"minMaf": 0.25, "minMac": 1}  # S = 1: maf is 0 or 0.5, nothing is missing, p is 1
COHORT = {"minMaf": 0.05, "maxMaf": 0.2, "minMac": 40, "maxMissing": 0.1, "hwe": 1e-6}


def singles(criteria):
    return [{k: v} for k, v in criteria.items()]


def cohort_vcf():
    """the CLI cases' file: two generated pieces under one header, 400 samples"""
    return vcfgen.gen_vcf(41, 3000, 400, weird=0.02) + vcfgen.gen_vcf(42, 1500, 400, weird=0.02).split(b"\n", 3)[3]


@functools.lru_cache(maxsize=None)
def case_input(name):
    import gtmask
    import pairtable as pt
    import samplecut
    if name.startswith("rare"):
        return pt.rare_vcf(int(name[4:]))
    if name.startswith("tile"):
        return pt.tile_vcf(int(name[4:]))
    if name == "masked13":  # what --minGQ 20 makes of fuzz13
        return gtmask.mask_vcf(pt.fuzz_vcf(13), MASK_GQ, 0)
    if name == "cut300":    # what --keepSamples makes of rare300
        return samplecut.cut_vcf(pt.rare_vcf(300), CUT_KEEP)
    return {"short": pt.short_list_limit_vcf, "sweep": hwe_sweep_vcf, "fuzz13": lambda: pt.fuzz_vcf(13),
            "one": lambda: pt.tiny_vcf(1), "cohort": cohort_vcf}[name]()


MASK_GQ = 20
CUT_KEEP = sorted(random.Random(9200).sample(range(300), 150))
CASES = {
    "rare63": [RARE], "rare64": [RARE], "rare65": [RARE], "rare300": [WIDE] + singles(RARE), "short": [RARE, WIDE],
    "tile1": [TILE, TILE_DROPS], "tile63": [TILE], "tile64": [TILE], "tile65": [TILE], "tile130": [TILE],
    "sweep": [SWEEP] + singles(SWEEP), "fuzz13": [FUZZ13], "masked13": [MASKED13], "cut300": [WIDE],
    "one": [ONE_SAMPLE, {"maxMaf": 0.25}], "cohort": [COHORT],
}
