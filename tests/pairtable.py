"""--relatedness: the expected pair tables and file text, built from the oracle's TSV of the same bytes (numpy only).

A row of the TSV names samples in its heterozygotes / homozygotes / missingGenos columns: three 0/1 matrices H, O, M
(rows x samples).  With C = H + O + M the tables are HH = H^T H, OC = O^T C, HM = H^T M; the products are formed in
float32, which is exact as long as every count stays below 2^24 (asserted).  Test infrastructure only."""
import random

import numpy as np

import vcfgen

COLUMNS = ["sample1", "sample2", "hetHet", "ibs0", "het1", "het2", "kinship"]
BASE_HEADER = ["chrom", "pos", "type", "ref", "alt", "trTv", "heterozygotes", "heterozygosity", "homozygotes", "homozygosity",
               "missingGenos", "missingness", "ac", "an", "sampleMaf"]


def sample_names(vcf):
    for ln in vcf.split(b"\n"):
        if ln.startswith(b"#CHROM"):
            return [x.decode() for x in ln.rstrip(b"\r").split(b"\t")[9:]]
    return []


def matrices(tsv_body, names, cfg=None):
    """(H, O, M) uint8 matrices, rows x samples, of a TSV body (no header line)"""
    cfg = cfg or {}
    delim, empty = cfg.get("fieldDelimiter", ";").encode(), cfg.get("emptyField", "!").encode()
    cols = [BASE_HEADER.index(x) for x in ("heterozygotes", "homozygotes", "missingGenos")]
    index = {nm.encode(): i for i, nm in enumerate(names)}
    assert len(index) == len(names), "sample names repeat"
    rows = [r for r in tsv_body.split(b"\n") if r]
    mats = [np.zeros((len(rows), len(names)), dtype=np.uint8) for _ in range(3)]
    for r, row in enumerate(rows):
        f = row.split(b"\t")
        for q, col in enumerate(cols):
            if f[col] != empty:
                mats[q][r, [index[x] for x in f[col].split(delim)]] = 1
    return tuple(mats)


def tables(H, O, M):
    """(3, S, S) uint64: HH, OC, HM"""
    assert H.shape[0] < (1 << 24), "float32 products would not be exact"
    assert int((H.astype(np.uint16) + O + M).max(initial=0)) <= 1, "a sample is named in two lists of one row"
    h, o, m = (x.astype(np.float32) for x in (H, O, M))
    c = h + o + m
    return np.stack([h.T @ h, o.T @ c, h.T @ m]).astype(np.uint64)


def derive(t, i, j):
    """(hetHet, ibs0, het1, het2, num, den) of the pair i < j, Python ints"""
    hh, oc, hm = t
    het_het = int(hh[i, j])
    ibs0 = (int(oc[i, i]) - int(oc[i, j])) + (int(oc[j, j]) - int(oc[j, i]))
    het1 = int(hh[i, i]) - int(hm[i, j])
    het2 = int(hh[j, j]) - int(hm[j, i])
    return het_het, ibs0, het1, het2, 2 * het_het - 4 * ibs0 - het1 - het2, 4 * min(het1, het2)


def file_text(t, names, empty="!"):
    """the --relatedness file of the tables"""
    out = ["\t".join(COLUMNS)]
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            het_het, ibs0, het1, het2, num, den = derive(t, i, j)
            kin = empty if den == 0 else "%.3G" % (0.5 + num / den)
            out.append("%s\t%s\t%d\t%d\t%d\t%d\t%s" % (names[i], names[j], het_het, ibs0, het1, het2, kin))
    return ("\n".join(out) + "\n").encode()


def expected(oracle_run, vcf, cfg=None):
    """(tables, file text) of a VCF through the oracle (oracle_run: oracle_lib.run)"""
    rc, body, _, _ = oracle_run(vcf, cfg)
    assert rc == 0
    names = sample_names(vcf)
    t = tables(*matrices(body, names, cfg))
    return t, file_text(t, names, (cfg or {}).get("emptyField", "!"))


# ---- inputs

FUZZ = [(11, 600, 17, False, "\n"), (12, 500, 300, False, "\n"), (13, 400, 300, True, "\r\n"), (14, 300, 70, False, "\n")]


def fuzz_vcf(seed):
    """the vcfgen.gen_vcf inputs of the table cases, by seed"""
    for s, n_lines, ns, fmt_extra, eol in FUZZ:
        if s == seed:
            return vcfgen.gen_vcf(s, n_lines, ns, fmt_extra, eol=eol)
    raise KeyError(seed)


RARE_SAMPLES = [63, 64, 65, 129, 300]


def rare_vcf(ns, n_lines=240, seed=None):
    """lines that few samples carry (a short class list on the streaming path) among lines that a quarter to a half of
    the cohort carries (a dense map): SNP, multiallelic and MNP lines; het, hom, missing, haploid and polyploid calls"""
    rng = random.Random(7000 + ns if seed is None else seed)
    names = ["R%04d" % i for i in range(ns)]
    out = [vcfgen.header(ns, names=names)]
    odd = ["./.", ".|.", "1", "0", "0|1|1", "1|.", "."]
    pos = 500
    for _ in range(n_lines):
        pos += rng.randint(1, 40)
        kind = rng.random()
        if kind < 0.08:
            ref, alt = "ACG", "TCA"
        elif kind < 0.25:
            ref, alt = "A", "C,G"
        else:
            ref = rng.choice("ACGT")
            alt = rng.choice([b for b in "ACGT" if b != ref])
        n_alts = alt.count(",") + 1
        gts = ["0|0"] * ns
        n_car = rng.randint(1, 6) if rng.random() < 0.7 else rng.randint(ns // 4, ns // 2)
        for _ in range(n_car):
            s = rng.randrange(ns)
            if rng.random() < 0.2:
                gts[s] = rng.choice(odd)
            else:
                gts[s] = "%d%s%d" % (rng.randint(0, n_alts), rng.choice("|/"), rng.randint(0, n_alts))
        filt = rng.choice(["PASS", "PASS", ".", "q10"])
        out.append("\t".join(["chr1", str(pos), ".", ref, alt, "50", filt, "DP=10", "GT"] + gts) + "\n")
    return "".join(out).encode()


TILE_ROWS = [1, 63, 64, 65, 130]


def tile_vcf(n_rows, ns=70):
    """exactly n_rows rows: plain PASS SNP lines, each with at least one carrier, a third of the cohort called otherwise"""
    rng = random.Random(8000 + n_rows)
    out = [vcfgen.header(ns)]
    for k in range(n_rows):
        gts = [rng.choice(["0|0", "0|0", "0|1", "1|1", "./.", "1|0"]) for _ in range(ns)]
        gts[rng.randrange(ns)] = rng.choice(["0|1", "1|1"])
        out.append("\t".join(["chr2", str(100 + 3 * k), ".", "A", "G", "50", "PASS", ".", "GT"] + gts) + "\n")
    return "".join(out).encode()


def snp_line(pos, gts, ref="C", alt="T"):
    return "\t".join(["chr3", str(pos), ".", ref, alt, "50", "PASS", ".", "GT"] + gts) + "\n"


def short_list_limit_vcf(ns=300):
    """a short class list at its limit -- the carriers of one row fill 15 map bytes x 4 adjacent samples -- and a row with 16
    non-zero map bytes, which no longer fits one; a few ordinary rows around them.  Every call is phased, missing ones
    too: a line that mixes separators leaves the streaming kernel's list mode for the general scan and a dense map"""
    rng = random.Random(8100)
    out = [vcfgen.header(ns)]
    calls = ["0|1", "1|1", ".|.", "1|0"]
    for pos, n_bytes in ((100, 15), (200, 16), (300, 15), (400, 1)):
        gts = ["0|0"] * ns
        for b in rng.sample(range(ns // 4), n_bytes):
            for q in range(4):
                gts[4 * b + q] = rng.choice(calls)
        out.append(snp_line(pos, gts))
    for k in range(20):
        gts = ["0|0"] * ns
        for s in rng.sample(range(ns), rng.randint(1, 5)):
            gts[s] = rng.choice(calls)
        out.append(snp_line(500 + 10 * k, gts))
    return "".join(out).encode()


def never_het_vcf(ns=9, n_lines=40):
    """sample 0 is never het (0|0 or 1|1 on every row): den == 0 for its pairs"""
    rng = random.Random(8200)
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        gts = [rng.choice(["0|0", "0|1", "1|1", "./.", "1|0"]) for _ in range(ns)]
        gts[0] = rng.choice(["0|0", "1|1"])
        gts[1 + k % (ns - 1)] = "0|1"
        out.append(snp_line(100 + 5 * k, gts))
    return "".join(out).encode()


def half_missing_vcf(ns=12, n_lines=60):
    """sample 1 is missing on every other row: het1 of a pair (i, 1) is below the het count of i"""
    rng = random.Random(8300)
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        gts = [rng.choice(["0|0", "0|1", "1|1", "1|0"]) for _ in range(ns)]
        gts[1] = "./." if k % 2 else rng.choice(["0|1", "1|1"])
        gts[0] = "0|1"
        out.append(snp_line(100 + 5 * k, gts))
    return "".join(out).encode()


def tiny_vcf(ns, n_lines=30):
    """S = 1 and S = 2"""
    rng = random.Random(8400 + ns)
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        gts = [rng.choice(["0|0", "0|1", "1|1", "./.", "1|0"]) for _ in range(ns)]
        out.append(snp_line(100 + 5 * k, gts))
    return "".join(out).encode()


def seeded_inputs():
    """every seeded (not crafted) input of the table cases: {name: bytes}"""
    d = {"fuzz%d" % s[0]: fuzz_vcf(s[0]) for s in FUZZ}
    d.update({"rare%d" % ns: rare_vcf(ns) for ns in RARE_SAMPLES})
    return d
