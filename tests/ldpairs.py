"""--ld / --ldPrune: the expected pairs, table and prune lists, built from the oracle's TSV of the same bytes.

Written from the definitions in include/bvcf.h (bvcf_enable_ld) and shares no code with the library: the H / O / M
matrices come from the TSV through pairtable.matrices, the six counts are numpy integers, the predicate is Python
integers, r2 is Python floats in the stated order of operations.  Test infrastructure only."""
import random

import numpy as np

import pairtable as pt
import vcfgen

HEADER = b"chrom\tpos1\tref1\talt1\tpos2\tref2\talt2\tn\tr2\tdir\n"
T6_ONE = 10 ** 6


def rows_of(tsv_body):
    """[(chrom, pos, ref, alt)] of a TSV body (no header line), bytes"""
    out = []
    for r in tsv_body.split(b"\n"):
        if r:
            f = r.split(b"\t")
            out.append((f[0], f[1], f[3], f[4]))
    return out


def genotypes(H, O, M):
    """(G, V): int64 genotypes 0 / 1 / 2 and the 0/1 matrix of called samples"""
    assert int((H.astype(np.uint16) + O + M).max(initial=0)) <= 1, "a sample is named in two lists of one row"
    return H.astype(np.int64) + 2 * O.astype(np.int64), 1 - M.astype(np.int64)


def six_counts(ga, va, gb, vb):
    """n, sa, sb, saa, sbb, sab of two rows (int64 vectors of genotypes and called flags), Python ints"""
    v = va * vb
    return [int(x) for x in (v.sum(), (ga * v).sum(), (gb * v).sum(), (ga * ga * v).sum(), (gb * gb * v).sum(), (ga * gb * v).sum())]


def moments(k):
    n, sa, sb, saa, sbb, sab = (int(x) for x in k)
    return n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb


def in_ld(k, t6):
    c, va, vb = moments(k)
    return va > 0 and vb > 0 and c * c * T6_ONE >= t6 * va * vb


def r2_of(k):
    c, va, vb = moments(k)
    return (float(c) * float(c)) / (float(va) * float(vb))


def bed_rows(H, O, M):
    """the rows in PLINK .bed code, uint8 (rows, ceil(S / 4)): 0 hom ALT, 1 missing, 2 het, 3 hom REF; pad bits 0"""
    n, S = H.shape
    code = np.full((n, S), 3, dtype=np.uint8)
    code[H == 1] = 2
    code[O == 1] = 0
    code[M == 1] = 1
    rb = (S + 3) // 4
    pad = np.zeros((n, 4 * rb), dtype=np.uint8)
    pad[:, :S] = code
    q = pad.reshape(n, rb, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def band_counts(G, V, window, block=512):
    """yields (b0, K) per block of rows: K int64 (6, rows of the block, window) -- K[:, i, d - 1] = the six counts of the
    pair (b0 + i - d, b0 + i); float32 products, exact below 2^24 (asserted)"""
    n, S = G.shape
    assert 4 * S < (1 << 24)
    v = V.astype(np.float32)
    gv = (G * V).astype(np.float32)
    ggv = (G * G * V).astype(np.float32)
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        a0 = max(0, b0 - window)
        # [a, b] products of the rows a in [a0, b1) with the rows b in [b0, b1)
        full = np.stack([v[a0:b1] @ v[b0:b1].T, gv[a0:b1] @ v[b0:b1].T, v[a0:b1] @ gv[b0:b1].T, ggv[a0:b1] @ v[b0:b1].T,
                         v[a0:b1] @ ggv[b0:b1].T, gv[a0:b1] @ gv[b0:b1].T]).astype(np.int64)
        K = np.zeros((6, b1 - b0, window), dtype=np.int64)
        for d in range(1, window + 1):
            i_lo = max(0, a0 + d - b0)  # rows b = b0 + i with b - d >= a0
            if i_lo >= b1 - b0:
                break
            i = np.arange(i_lo, b1 - b0)
            K[:, i, d - 1] = full[:, b0 + i - d - a0, i]
        yield b0, K


def events_of(H, O, M, chroms, window, t6):
    """uint32 (n, 8): b, d, n, sa, sb, saa, sbb, sab of every pair in LD of the run, by b, then by a ascending.  The
    predicate is decided in Python integers; float64 only sorts out the pairs that are far from the threshold."""
    G, V = genotypes(H, O, M)
    n = G.shape[0]
    ids = {}
    chrom_id = np.array([ids.setdefault(c, len(ids)) for c in chroms], dtype=np.int64)
    out = []
    # (a block's products cover (block + window) x block pairs for a band of window x block: short blocks for wide cohorts)
    for b0, K in band_counts(G, V, window, block=max(32, min(512, (1 << 17) // G.shape[1]))):
        nb = K.shape[1]
        kn, sa, sb, saa, sbb, sab = (K[q].astype(np.float64) for q in range(6))
        c = kn * sab - sa * sb
        va, vb = kn * saa - sa * sa, kn * sbb - sb * sb
        lhs, rhs = c * c * float(T6_ONE), float(t6) * va * vb
        b = b0 + np.arange(nb)[:, None]
        d = np.arange(1, window + 1)[None, :]
        ok = (d <= b) & (va > 0) & (vb > 0)
        ok &= chrom_id[np.clip(b - d, 0, n - 1)] == chrom_id[b]
        near = ok & (np.abs(lhs - rhs) <= 1e-9 * (lhs + rhs))
        yes = ok & ~near & (lhs > rhs)
        for i, j in zip(*np.nonzero(near)):
            if in_ld(K[:, i, j], t6):
                yes[i, j] = True
        for i in np.nonzero(yes.any(axis=1))[0]:
            for j in np.nonzero(yes[i])[0][::-1]:
                out.append([b0 + i, j + 1] + K[:, i, j].tolist())
    return np.array(out, dtype=np.uint32).reshape(-1, 8)


def table_text(events, rows):
    out = [HEADER]
    for e in events.tolist():
        b, d, k = e[0], e[1], e[2:]
        ra, rb = rows[b - d], rows[b]
        c = moments(k)[0]
        r2 = r2_of(k)
        out.append(b"\t".join([ra[0], ra[1], ra[2], ra[3], rb[1], rb[2], rb[3], b"%d" % k[0],
                               (b"0" if r2 == 0.0 else ("%.3G" % r2).encode()), b"+" if c > 0 else b"-" if c < 0 else b"0"]) + b"\n")
    return b"".join(out)


def prune(events, n_rows):
    """kept flags of the greedy walk in file order: b is pruned iff some pair (a, b) in LD has a kept a"""
    kept = np.ones(n_rows, dtype=bool)
    by_b = {}
    for b, d in events[:, :2].tolist():
        by_b.setdefault(b, []).append(b - d)
    for b in range(n_rows):
        if any(kept[a] for a in by_b.get(b, ())):
            kept[b] = False
    return kept


def lists_text(kept, rows):
    loci = [b":".join(r) + b"\n" for r in rows]
    return b"".join(x for x, k in zip(loci, kept) if k), b"".join(x for x, k in zip(loci, kept) if not k)


def expected_from_body(tsv_body, names, window, t6, cfg=None, with_table=True):
    """-> dict(rows, events, kept, table, prune_in, prune_out, bed): names = the header's sample names of the body's file"""
    rows = rows_of(tsv_body)
    if not names:
        return {"rows": [], "events": np.zeros((0, 8), dtype=np.uint32), "kept": np.zeros(0, dtype=bool), "table": HEADER,
                "prune_in": b"", "prune_out": b"", "bed": np.zeros((0, 0), dtype=np.uint8), "hom": None}
    names = [nm.replace(".", "_") for nm in names]
    H, O, M = pt.matrices(tsv_body, names, cfg)
    ev = events_of(H, O, M, [r[0] for r in rows], window, t6)
    kept = prune(ev, len(rows))
    pin, pout = lists_text(kept, rows)
    return {"rows": rows, "events": ev, "kept": kept, "table": table_text(ev, rows) if with_table else None, "prune_in": pin,
            "prune_out": pout, "bed": bed_rows(H, O, M), "hom": (H, O, M)}


def expected(oracle_run, vcf, window, t6, cfg=None, with_table=True):
    rc, body, log, _ = oracle_run(vcf, cfg)
    assert rc == 0
    return expected_from_body(body, pt.sample_names(vcf), window, t6, cfg, with_table), body, log


def batch_events(events, lo, hi):
    """the events a device reports for the batch of the run's rows [lo, hi): both rows inside, b local to the batch"""
    b, a = events[:, 0].astype(np.int64), events[:, 0].astype(np.int64) - events[:, 1]
    e = events[(b >= lo) & (b < hi) & (a >= lo)].copy()
    e[:, 0] -= lo
    return e


def loci_of(rows):
    return [b"\t".join(r) for r in rows]


def coverage(want, window):
    """what an input exercises, from the reference alone -> set of names"""
    H, O, M = want["hom"]
    G, V = genotypes(H, O, M)
    rows, ev = want["rows"], want["events"]
    n = len(rows)
    seen = set()
    in_ld_pairs = {(b - d, b) for b, d in ev[:, :2].tolist()}
    if in_ld_pairs:
        seen.add("in_ld")
    for e in ev.tolist():
        if moments(e[2:])[0] < 0:
            seen.add("negative_c")
        c, va, vb = moments(e[2:])
        if c * c == va * vb:
            seen.add("exact_at_1")
    for b in range(n):
        for a in range(max(0, b - window), b):
            same = rows[a][0] == rows[b][0]
            if not same:
                seen.add("chrom_change_in_window")
                continue
            if (a, b) in in_ld_pairs:
                continue
            seen.add("not_in_ld")
            k = six_counts(G[a], V[a], G[b], V[b])
            c, va, vb = moments(k)
            whole_a = six_counts(G[a], V[a], G[a], V[a])
            if va == 0 and moments(whole_a)[1] > 0 and k[0] > 0:
                seen.add("va0_by_missing")
    loci = [r[0] + b":" + r[1] for r in rows]
    if len(set(loci)) < len(loci):
        seen.add("multiallelic")
    # a kept, b pruned by a, c in LD with b and with no kept row -> kept
    kept = want["kept"]
    partners = {}
    for a, b in in_ld_pairs:
        partners.setdefault(b, []).append(a)
    for c_row, ps in partners.items():
        if kept[c_row] and any(not kept[p] and any(kept[a] for a in partners.get(p, ())) for p in ps):
            seen.add("rescued")
    return seen


NEEDED = {"in_ld", "not_in_ld", "negative_c", "exact_at_1", "chrom_change_in_window", "va0_by_missing", "multiallelic", "rescued"}


def _gt(g, phased=True):
    sep = "|" if phased else "/"
    return {0: "0" + sep + "0", 1: "0" + sep + "1", 2: "1" + sep + "1", -1: "." + sep + "."}[g]


def ld_vcf(seed, ns, n_rows, specials=True, miss=0.03, carrier=0.3):
    """n_rows + a few rows of a cohort of ns samples with LD between neighbours: a row is its predecessor with a few calls
    redrawn, a fresh draw, or the predecessor's complement (a negative c); raw "1" lines next to "chr1" lines, then
    "chr2"; with specials: two identical rows (r2 = 1 exactly), a row missing wherever its predecessor is not REF (va = 0
    through missing calls only) and a multiallelic line"""
    rng = random.Random(seed)
    out = [vcfgen.header(ns)]

    def fresh():
        g = [rng.choice([0, 1, 2]) if rng.random() < carrier else 0 for _ in range(ns)]
        g[rng.randrange(ns)] = rng.choice([1, 2])
        return g

    def line(chrom, pos, g, ref="A", alt="G", fmt=None):
        calls = fmt or [_gt(x) for x in g]
        return "\t".join([chrom, str(pos), ".", ref, alt, "50", "PASS", ".", "GT"] + calls) + "\n"

    cur = fresh()
    pos = 1000
    for k in range(n_rows):
        chrom = "1" if k < n_rows // 3 else "chr1" if k < (2 * n_rows) // 3 else "chr2"
        r = rng.random()
        if r < 0.12:
            cur = fresh()
        elif r < 0.24 and ns > 1:
            cur = [2 - x for x in cur]
            if not any(cur):
                cur = fresh()
        else:
            cur = [rng.choice([0, 1, 2]) if rng.random() < 0.08 else x for x in cur]
            if not any(cur):
                cur = fresh()
        g = [-1 if (rng.random() < miss and ns > 1) else x for x in cur]
        if not any(x > 0 for x in g):
            g = list(cur)
        pos += rng.randint(1, 40)
        out.append(line(chrom, pos, g))
        if specials and k == n_rows // 6:
            pos += 5
            out.append(line(chrom, pos, g, ref="C", alt="T"))  # the same calls again: r2 = 1 exactly
            if ns >= 4:
                # missing wherever the row before is not REF, carriers among the rest
                h = [-1 if x != 0 else rng.choice([0, 0, 1, 2]) for x in g]
                free = [i for i, x in enumerate(g) if x == 0]
                if len(free) >= 2:
                    h[free[0]], h[free[1]] = 1, 0
                    pos += 5
                    out.append(line(chrom, pos, h, ref="G", alt="A"))
            # a multiallelic line: ALT 1 as the row before has it, ALT 2 in a few samples that are REF there
            calls = [_gt(x) for x in g]
            for i in [i for i, x in enumerate(g) if x == 0][:3]:
                calls[i] = "0|2"
            if any(c == "0|2" for c in calls):
                pos += 5
                out.append(line(chrom, pos, g, ref="T", alt="C,G", fmt=calls))
    return "".join(out).encode()


def exact_third_vcf():
    """the example of the definitions: g_a = (0, 0, 1, 1), g_b = (0, 0, 0, 1): c = 2, va = 4, vb = 3, r2 = 1/3 -- in LD at
    0.333333, not at 0.333334"""
    out = [vcfgen.header(4)]
    for pos, g in ((100, (0, 0, 1, 1)), (200, (0, 0, 0, 1))):
        out.append("\t".join(["chr7", str(pos), ".", "A", "G", "50", "PASS", ".", "GT"] + [_gt(x) for x in g]) + "\n")
    return "".join(out).encode()


# cohort sizes of the GPU tests: word (16 samples), lane, chunk (512 samples) edges and a partial last byte
GPU_SAMPLES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300]
GPU_ROWS = [1, 2, 15, 16, 17, 63, 64, 65, 130]
GPU_WINDOWS = [1, 2, 63, 64, 65, 200, 512]


def seeded_inputs():
    """name -> (vcf, window): the inputs the GPU tests compare byte for byte, with every condition of NEEDED in each of the
    first three (test_ld_cpu.py checks that with the oracle alone)"""
    return {"ld40": (ld_vcf(7001, 40, 150), 50), "ld129": (ld_vcf(7002, 129, 120), 20), "ld300": (ld_vcf(7003, 300, 140), 64)}
