"""--mendel / --mendelErrors: the expected per-trio table and event list, built from the oracle's TSV of the same bytes
(numpy and Python only).

The oracle does not know the flags.  A row of its TSV names samples in heterozygotes / homozygotes / missingGenos
(pairtable.matrices); a sample's class in the row is the list that names it: ref (none), het, hom, missing.  Per
(row, trio) with the classes c, f, m of child, father and mother:

    uninformative  one of the three is missing
    consistent     the child's ALT count d(c) -- 0 / 1 / 2 for ref / het / hom -- is a + b for an allele count a the father can
                   transmit and a b the mother can: ref {0}, het {0, 1}, hom {1}
    denovo         otherwise, with both parents ref
    error          otherwise

The verdict here enumerates the transmissions; the .fam parser is written from the rules in include/bvcf.h.  Neither
comes from the library.  Test infrastructure only."""
import random
import re

import numpy as np

import pairtable as pt
import vcfgen

REF, HET, HOM, MISSING = 0, 1, 2, 3
CLASS_NAMES = ["ref", "het", "hom", "missing"]
UNINFORMATIVE, CONSISTENT, DENOVO, ERROR = 0, 1, 2, 3
MENDEL_HEADER = b"child\tfather\tmother\tinformative\terrors\tdenovo\terrorRate\n"
ERRORS_HEADER = b"chrom\tpos\tref\talt\tchild\tfather\tmother\tchildClass\tfatherClass\tmotherClass\tkind\n"

# reasons a .fam fails (the numbers of BVCF_FAM_*)
FAM_SHORT_LINE, FAM_DUP_IID, FAM_AMBIGUOUS, FAM_SAME_SAMPLE = 1, 2, 3, 4


class FamError(Exception):
    def __init__(self, why, line, iid):
        Exception.__init__(self, "fam line %d: reason %d (%r)" % (line, why, iid))
        self.why, self.line, self.iid = why, line, iid


def transmits(cls):
    """the ALT allele counts a parent of this class can hand on"""
    return {REF: {0}, HET: {0, 1}, HOM: {1}}[cls]


def verdict(c, f, m):
    if MISSING in (c, f, m):
        return UNINFORMATIVE
    dose = {REF: 0, HET: 1, HOM: 2}[c]
    if any(a + b == dose for a in transmits(f) for b in transmits(m)):
        return CONSISTENT
    return DENOVO if (f, m) == (REF, REF) else ERROR


INFORMATIVE_TRIPLES = [(c, f, m) for c in range(3) for f in range(3) for m in range(3)]


def parse_fam(text, names):
    """text: the file's bytes; names: the (kept) sample names as --sample writes them, bytes, header order.
    -> [(child, father, mother)] as indices into names, by child; FamError on the first line that breaks a rule"""
    cols = {}
    for i, nm in enumerate(names):
        cols.setdefault(nm, []).append(i)
    seen, trios = set(), []
    for n, raw in enumerate(text.split(b"\n"), 1):
        if raw.endswith(b"\r"):
            raw = raw[:-1]
        f = [x for x in re.split(rb"[ \t]+", raw) if x]
        if not f:
            continue
        if len(f) < 4:
            raise FamError(FAM_SHORT_LINE, n, None)
        iid = f[1]
        if iid not in cols:
            continue  # not a sample of this run
        if len(cols[iid]) > 1:
            raise FamError(FAM_AMBIGUOUS, n, iid)
        if iid in seen:
            raise FamError(FAM_DUP_IID, n, iid)
        seen.add(iid)
        who = [cols[iid][0]]
        for parent in f[2:4]:
            if parent == b"0" or parent not in cols:
                who.append(None)
                continue
            if len(cols[parent]) > 1:
                raise FamError(FAM_AMBIGUOUS, n, iid)
            who.append(cols[parent][0])
        if None in who:
            continue
        if len(set(who)) < 3:
            raise FamError(FAM_SAME_SAMPLE, n, iid)
        trios.append(tuple(who))
    return sorted(trios)


def normalized(names):
    """the names as --sample writes them (parse.NormalizeHeader: '.' -> '_')"""
    return [nm.replace(".", "_") for nm in names]


def classes_of(H, O, M):
    """(rows, S) uint8 of REF / HET / HOM / MISSING"""
    assert int((H.astype(np.uint16) + O + M).max(initial=0)) <= 1, "a sample is named in two lists of one row"
    cls = np.zeros(H.shape, dtype=np.uint8)
    cls[H == 1] = HET
    cls[O == 1] = HOM
    cls[M == 1] = MISSING
    return cls


_VERDICT = np.array([[[verdict(c, f, m) for m in range(4)] for f in range(4)] for c in range(4)], dtype=np.uint8)


def verdicts(cls, trios):
    """(rows, T) uint8 of verdicts, and the (rows, T, 3) classes"""
    if not len(trios):
        return np.zeros((cls.shape[0], 0), dtype=np.uint8), np.zeros((cls.shape[0], 0, 3), dtype=np.uint8)
    t = np.asarray(trios, dtype=np.int64)
    cfm = np.stack([cls[:, t[:, q]] for q in range(3)], axis=2)
    return _VERDICT[cfm[:, :, 0], cfm[:, :, 1], cfm[:, :, 2]], cfm


def counts_of(v):
    """(T, 3) informative, errors (de novo included), de novo"""
    return np.stack([(v != UNINFORMATIVE).sum(0), (v >= DENOVO).sum(0), (v == DENOVO).sum(0)], axis=1).astype(np.uint64)


def events_of(v, cfm):
    """(n, 5) row, trio, c, f, m of every de novo / error verdict: by row, then by trio"""
    rows, ts = np.nonzero(v >= DENOVO)
    return np.concatenate([rows[:, None], ts[:, None], cfm[rows, ts]], axis=1).astype(np.uint32).reshape(-1, 5)


def mendel_text(counts, trios, names, empty="!"):
    out = [MENDEL_HEADER]
    for (c, f, m), (inf, err, dn) in zip(trios, counts.tolist()):
        rate = empty if inf == 0 else ("0" if err == 0 else "%.3G" % (err / inf))
        out.append(("%s\t%s\t%s\t%d\t%d\t%d\t%s\n" % (names[c], names[f], names[m], inf, err, dn, rate)).encode())
    return b"".join(out)


def errors_text(events, tsv_body, trios, names):
    rows = [r for r in tsv_body.split(b"\n") if r]
    out = [ERRORS_HEADER]
    for r, t, c, f, m in events.tolist():
        col = rows[r].split(b"\t")
        who = [names[i].encode() for i in trios[t]]
        kind = b"denovo" if (f, m) == (REF, REF) else b"error"
        out.append(b"\t".join([col[0], col[1], col[3], col[4]] + who + [CLASS_NAMES[x].encode() for x in (c, f, m)] + [kind]) + b"\n")
    return b"".join(out)


def expected_from_body(tsv_body, names, fam, cfg=None, with_errors_text=True):
    """names: the header's sample names (str) of the TSV body's file -> dict(trios, counts, events, verdicts, mendel, errors,
    names); with_errors_text=False leaves "errors" out (a list of hundreds of thousands of lines: errors_text on a slice)"""
    cfg = cfg or {}
    names = normalized(names)
    trios = parse_fam(fam, [n.encode() for n in names])
    if names:
        cls = classes_of(*pt.matrices(tsv_body, names, cfg))
    else:
        cls = np.zeros((0, 0), dtype=np.uint8)
    v, cfm = verdicts(cls, trios)
    counts, events = counts_of(v), events_of(v, cfm)
    return {"trios": trios, "counts": counts, "events": events, "verdicts": v, "names": names,
            "mendel": mendel_text(counts, trios, names, cfg.get("emptyField", "!")),
            "errors": errors_text(events, tsv_body, trios, names) if with_errors_text else None}


def expected(oracle_run, vcf, fam, cfg=None, with_errors_text=True):
    """(counts table, --mendel text, --mendelErrors text) plus everything else in a dict, the TSV body and the log of a VCF
    through the oracle (oracle_run: oracle_lib.run)"""
    rc, body, log, _ = oracle_run(vcf, cfg)
    assert rc == 0
    return expected_from_body(body, pt.sample_names(vcf), fam, cfg, with_errors_text), body, log


def coverage(v, cfm):
    """the verdict kinds present and the informative triples seen"""
    kinds = set(np.unique(v).tolist())
    inf = cfm[v != UNINFORMATIVE].reshape(-1, 3)
    return kinds, {tuple(x) for x in np.unique(inf, axis=0).tolist()} if len(inf) else set()


# ---- pedigrees

def fam_of(trios, names, extra_lines=(), sep="\t", eol="\n"):
    """a .fam naming every sample once: the trios' children with their parents, everybody else a founder"""
    child = {c: (f, m) for c, f, m in trios}
    out = []
    for i, nm in enumerate(names):
        f, m = child.get(i, (None, None))
        out.append(sep.join(["F1", nm, names[f] if f is not None else "0", names[m] if m is not None else "0", "0", "-9"]))
    out.extend(extra_lines)
    return (eol.join(out) + eol).encode()


def block_trios(n_trios, ns=None, child_first=False):
    """trio t = samples (3t, 3t + 1, 3t + 2) as (father, mother, child) -- or (child, father, mother) positions with
    child_first, where the child's header position precedes its parents'"""
    if child_first:
        return [(3 * t, 3 * t + 1, 3 * t + 2) for t in range(n_trios)]
    return [(3 * t + 2, 3 * t, 3 * t + 1) for t in range(n_trios)]


def random_trios(ns, n_trios, seed):
    """a random pedigree over ns samples: distinct children; parents drawn from everybody, so a sample can be a child in one
    trio and a parent in others, and children share parents"""
    rng = random.Random(seed)
    trios = []
    for c in rng.sample(range(ns), min(n_trios, ns)):
        f, m = rng.sample([s for s in range(ns) if s != c], 2)
        trios.append((c, f, m))
    return sorted(trios)


# ---- inputs

GT_OF = {0: "0|0", 1: "0|1", 2: "1|1"}


def pedigree_vcf(ns, n_trios, n_rows, seed, flip=0.02, miss=0.02, names=None, child_first=False):
    """inheritance simulated over block_trios(n_trios): rows that few founders carry (a short list on the streaming path)
    among rows a quarter of the cohort carries (a dense map); children draw one allele from each parent; flipped calls (the
    events) and missing calls at a small rate in the dense rows, one to four of them in the others.  All calls phased so that the streaming kernel keeps its list mode.
    -> (vcf bytes, trios)"""
    rng = random.Random(seed)
    trios = block_trios(n_trios, ns, child_first)
    assert 3 * n_trios <= ns
    children = {c: (f, m) for c, f, m in trios}
    out = [vcfgen.header(ns, names=names)]
    for k in range(n_rows):
        dense = k % 3 == 2
        dose = [0] * ns
        founders = [s for s in range(ns) if s not in children]
        if dense:
            for s in founders:
                if rng.random() < 0.25:
                    dose[s] = rng.choice([1, 1, 2])
        else:
            for s in rng.sample(founders, min(len(founders), rng.randint(1, 3))):
                dose[s] = rng.choice([1, 1, 2])
        for c, (f, m) in children.items():
            dose[c] = sum(rng.choice({0: [0], 1: [0, 1], 2: [1]}[dose[p]]) for p in (f, m))
        gts = [GT_OF[d] for d in dose]
        if dense:
            noisy = [s for s in range(ns) if rng.random() < miss + flip]
        else:  # (few enough that the row stays a short list: at most 3 + 3 + 4 samples are not 0|0)
            noisy = rng.sample(range(ns), min(ns, rng.randint(1, 4)))
        for s in noisy:
            if rng.random() * (miss + flip) < miss:
                gts[s] = ".|."
            else:
                gts[s] = GT_OF[rng.choice([d for d in range(3) if d != dose[s]])]
        if not any("1" in g for g in gts):
            gts[founders[0]] = "0|1"
        out.append("\t".join(["chr5", str(1000 + 7 * k), ".", "A", "G", "50", "PASS", ".", "GT"] + gts) + "\n")
    return "".join(out).encode(), trios


def triples_vcf(pad=10):
    """27 trios x 27 rows + extras: trio t shows informative triple (t + r) % 27 in row r, so every trio sees every triple;
    `pad` founders that are all ref keep the carriers few (short lists) in some rows, and three dense rows follow.
    -> (vcf, trios)"""
    n_trios = 27
    ns = 3 * n_trios + pad
    trios = block_trios(n_trios)
    out = [vcfgen.header(ns)]
    for r in range(27):
        gts = ["0|0"] * ns
        for t, (c, f, m) in enumerate(trios):
            cc, ff, mm = INFORMATIVE_TRIPLES[(t + r) % 27]
            gts[c], gts[f], gts[m] = GT_OF[cc], GT_OF[ff], GT_OF[mm]
        if r % 4 == 0:
            gts[0] = ".|."
        out.append(pt.snp_line(100 + 10 * r, gts))
    return "".join(out).encode(), trios


def all_errors_vcf(n_trios, n_rows):
    """every row an error for every trio: parents 0|0, children 1|1 -- n_rows * n_trios events from short lines
    -> (vcf, trios)"""
    ns = 3 * n_trios
    trios = block_trios(n_trios)
    gts = ["0|0"] * ns
    for c, f, m in trios:
        gts[c] = "1|1"
    out = [vcfgen.header(ns)]
    for k in range(n_rows):
        out.append(pt.snp_line(100 + 2 * k, gts))
    return "".join(out).encode(), trios


def child_listed_parents_not_vcf(ns=300):
    """short-list rows in which a child is the only carrier of its map byte region: its parents' map bytes are not listed
    (trio (8, 100, 200): three different map bytes), and rows in which only a parent is listed.  -> (vcf, trios)"""
    trios = [(8, 100, 200), (9, 101, 201), (150, 10, 290)]
    out = [vcfgen.header(ns)]
    pos = 100
    for carriers in ([(8, "0|1")], [(8, "1|1")], [(100, "1|1")], [(200, "0|1"), (8, "0|1")], [(9, "1|1"), (101, "0|1")],
                     [(150, "0|1"), (8, ".|.")], [(290, "1|1"), (10, "1|1")], [(150, "1|1"), (290, "0|1"), (10, ".|.")]):
        gts = ["0|0"] * ns
        for s, g in carriers:
            gts[s] = g
        out.append(pt.snp_line(pos, gts))
        pos += 10
    rng = random.Random(9901)
    for k in range(6):  # dense rows
        gts = [rng.choice(["0|0", "0|1", "1|1", "0|0", ".|."]) for _ in range(ns)]
        out.append(pt.snp_line(pos, gts))
        pos += 10
    return "".join(out).encode(), trios


CHUNK_TRIOS = [1, 63, 64, 65, 130]  # trio chunk edges; S = 3 T + 1
TILE_ROWS = [1, 63, 64, 65, 130]    # row tile edges


def chunk_vcf(n_trios):
    return pedigree_vcf(3 * n_trios + 1, n_trios, 40, 9500 + n_trios, flip=0.05, miss=0.05)


def tile_vcf(n_rows):
    return pedigree_vcf(70, 23, n_rows, 9600 + n_rows, flip=0.08, miss=0.05)


def fuzz_inputs():
    """{name: (vcf, fam)}: vcfgen.gen_vcf files (multiallelic, haploid, odd calls) with a random pedigree"""
    d = {}
    for seed in (11, 12, 14):
        vcf = pt.fuzz_vcf(seed)
        names = normalized(pt.sample_names(vcf))
        d["fuzz%d" % seed] = (vcf, fam_of(random_trios(len(names), max(2, len(names) // 3), 9700 + seed), names))
    return d


def gpu_inputs():
    """every (vcf, fam) the GPU cases run whose coverage test_mendel_cpu.py checks: {name: (vcf, fam)}"""
    d = dict(fuzz_inputs())
    for t in CHUNK_TRIOS[1:]:
        vcf, trios = chunk_vcf(t)
        d["chunk%d" % t] = (vcf, fam_of(trios, pt.sample_names(vcf)))
    for r in TILE_ROWS[2:]:
        vcf, trios = tile_vcf(r)
        d["tile%d" % r] = (vcf, fam_of(trios, pt.sample_names(vcf)))
    vcf, trios = pedigree_vcf(300, 90, 120, 9800)
    d["ped300"] = (vcf, fam_of(trios, pt.sample_names(vcf)))
    vcf, trios = triples_vcf()
    d["triples"] = (vcf, fam_of(trios, pt.sample_names(vcf)))
    return d
