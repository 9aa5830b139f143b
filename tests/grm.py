"""--grm: the expected integer tables and the three files' bytes, built from the oracle's TSV of the same bytes.

A row of the TSV names samples in its heterozygotes / homozygotes / missingGenos columns: 0/1 matrices H, O, M (rows x
samples, pairtable.matrices).  A sample's dosage is g = H + 2 O, missing where M.  Per row n = S - sum M, a = sum H + 2 sum O,
D = 2 a (2n - a); rows with D == 0 are skipped.  q(g) is the integer nearest to (2n g - 2a) 2^14 / sqrt(D), ties away from
zero, defined in integers: |q| is the largest m >= 0 with (2m - 1)^2 D <= 4 (2n g - 2a)^2 2^28.  T = Q^T Q, MM = M^T M,
N(i,j) = N - miss_i - miss_j + MM(i,j), A = T / (2^28 N(i,j)).  Everything here is Python integers or products that are
exact in float64 (asserted).  Test infrastructure only."""
import math
import random

import numpy as np

import pairtable as pt
import vcfgen

SHIFT = 14
ONE = 1 << (2 * SHIFT)  # A = T / (ONE * N)


def q_exact(n, a, g):
    """the quantised score, by the definition alone"""
    num = 2 * n * g - 2 * a
    D = 2 * a * (2 * n - a)
    assert D > 0
    if num == 0:
        return 0
    # (2m - 1)^2 D <= R  <=>  2m - 1 <= isqrt(R // D)
    m = (math.isqrt((4 * num * num * ONE) // D) + 1) // 2
    assert (2 * m - 1) ** 2 * D <= 4 * num * num * ONE < (2 * m + 1) ** 2 * D
    return m if num > 0 else -m


def limbs(q):
    """three balanced base-256 digits of q, each in [-128, 127]"""
    out = []
    for _ in range(3):
        d = ((q + 128) & 255) - 128
        out.append(d)
        q = (q - d) >> 8
    assert q == 0
    return out


def row_counts(H, O, M):
    """per row: n, a, D as int64 arrays"""
    S = H.shape[1]
    n = S - M.sum(axis=1, dtype=np.int64)
    a = H.sum(axis=1, dtype=np.int64) + 2 * O.sum(axis=1, dtype=np.int64)
    return n, a, 2 * a * (2 * n - a)


def row_scores(n, a, D):
    """(rows, 3) int64: q(0), q(1), q(2) of every row; zeros for a monomorphic row"""
    memo = {}
    out = np.zeros((len(n), 3), dtype=np.int64)
    for r in range(len(n)):
        if D[r] == 0:
            continue
        key = (int(n[r]), int(a[r]))
        if key not in memo:
            memo[key] = [q_exact(key[0], key[1], g) for g in range(3)]
        out[r] = memo[key]
    return out


def score_matrix(H, O, M, qs, D):
    """Q (rows x samples, int64) and the 0/1 matrix of missing calls, over the GRM rows only"""
    keep = D != 0
    H, O, M, qs = H[keep], O[keep], M[keep], qs[keep]
    none = (H == 0) & (O == 0) & (M == 0)
    Q = np.where(none, qs[:, 0:1], 0) + np.where(H == 1, qs[:, 1:2], 0) + np.where(O == 1, qs[:, 2:3], 0)
    return Q.astype(np.int64), M.astype(np.uint8)


def tables(H, O, M, chunk=4096):
    """(T int64 S x S, MM int64 S x S, N): exact.  Q is split at 11 bits so that every float64 product sum is an integer
    below 2^53"""
    assert int((H.astype(np.uint16) + O + M).max(initial=0)) <= 1, "a sample is named in two lists of one row"
    n, a, D = row_counts(H, O, M)
    Q, Mk = score_matrix(H, O, M, row_scores(n, a, D), D)
    rows, S = Q.shape
    assert rows < (1 << 20), "int64 T and the float64 limb products would not be exact"
    hh, hl, ll, mm = (np.zeros((S, S)) for _ in range(4))
    for lo in range(0, rows, chunk):
        q = Q[lo:lo + chunk]
        qh = (q >> 11).astype(np.float64)
        ql = (q & 2047).astype(np.float64)
        m = Mk[lo:lo + chunk].astype(np.float64)
        hh += qh.T @ qh
        hl += qh.T @ ql
        ll += ql.T @ ql
        mm += m.T @ m
    for x in (hh, hl, ll, mm):
        assert float(np.abs(x).max(initial=0)) < 2.0 ** 53
    hl = hl.astype(np.int64)
    T = (hh.astype(np.int64) << 22) + ((hl + hl.T) << 11) + ll.astype(np.int64)
    return T, mm.astype(np.int64), rows


def pair_rows(MM, N):
    """N(i,j) = N - miss_i - miss_j + MM(i,j)"""
    miss = np.diag(MM)
    return N - miss[:, None] - miss[None, :] + MM


def matrix(T, MM, N):
    """A as float64, before the rounding to float32: the correctly rounded double of T over the double 2^28 N(i,j)"""
    nij = pair_rows(MM, N)
    den = nij.astype(np.float64) * float(ONE)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(nij > 0, T.astype(np.float64) / den, 0.0), nij


def files(T, MM, N, names):
    """the bytes of PREFIX.grm.bin, .grm.N.bin and .grm.id"""
    A, nij = matrix(T, MM, N)
    i, j = np.tril_indices(len(names))
    ids = "".join("%s\t%s\n" % (nm, nm) for nm in names).encode()
    return A[i, j].astype("<f4").tobytes(), nij[i, j].astype(np.float64).astype("<f4").tobytes(), ids


def expected(oracle_run, vcf, cfg=None, row_mask=None):
    """((T, MM, N), (bin, N.bin, id), TSV body, log) of a VCF through the oracle (oracle_run: oracle_lib.run); row_mask: the
    rows of the body that stay (a gate, a list, regions)"""
    rc, body, log, _ = oracle_run(vcf, cfg)
    assert rc == 0
    names = pt.sample_names(vcf)
    H, O, M = pt.matrices(body, names, cfg)
    if row_mask is not None:
        keep = np.asarray(row_mask, dtype=bool)
        H, O, M = H[keep], O[keep], M[keep]
    t = tables(H, O, M) if names else (np.zeros((0, 0), np.int64), np.zeros((0, 0), np.int64), 0)
    return t, files(*t, names), body, log


def double_matrix(H, O, M):
    """the GRM in floating point, from unquantised z, with the terms of the quantisation bound: (A, B, nij) where
    B(i,j) = mean over the rows with both called of |z_i| + |z_j|"""
    n, a, D = row_counts(H, O, M)
    keep = D != 0
    H, O, M, n, a, D = H[keep], O[keep], M[keep], n[keep], a[keep], D[keep]
    g = H.astype(np.float64) + 2.0 * O
    z = (2.0 * n[:, None] * g - 2.0 * a[:, None]) / np.sqrt(D.astype(np.float64))[:, None]
    called = 1.0 - M
    z *= called
    nij = called.T @ called
    az = np.abs(z)
    s = az.T @ called
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(nij > 0, (z.T @ z) / nij, 0.0)
        B = np.where(nij > 0, (s + s.T) / nij, 0.0)
    return A, B, nij


# ---- inputs

SAMPLE_EDGES = [1, 15, 16, 17, 63, 64, 65, 300]


def edge_vcf(ns, n_lines=90):
    """MFMA tile, lane and stride edges: dense rows (a quarter to a half of the cohort carries them; every sample differs
    from every other somewhere, so a transposed block shows) and rare rows"""
    rng = random.Random(9400 + ns)
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        gts = ["0|0"] * ns
        n_car = rng.randint(1, 3) if k % 3 == 0 else max(1, rng.randint(ns // 4, max(ns // 2, 1)))
        for s in rng.sample(range(ns), min(n_car, ns)):
            gts[s] = rng.choice(["0|1", "1|1", "1|0", ".|.", "0|1"])
        if all(x in ("0|0", ".|.") for x in gts):
            gts[rng.randrange(ns)] = "0|1"
        out.append(pt.snp_line(100 + 7 * k, gts))
    return "".join(out).encode()


def all_missing_sample_vcf(ns=12, n_lines=50):
    """sample 2 is missing on every row (N(i,2) = 0 for every i), sample 1 on every other row"""
    rng = random.Random(9500)
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        gts = [rng.choice(["0|0", "0|0", "0|1", "1|1", "1|0"]) for _ in range(ns)]
        gts[0] = "0|1"
        gts[1] = ".|." if k % 2 else rng.choice(["0|1", "0|0"])
        gts[2] = ".|."
        out.append(pt.snp_line(100 + 5 * k, gts))
    return "".join(out).encode()


def monomorphic_vcf(ns=20):
    """rows every called sample is het in (kept: p = 1/2, every z is 0 ... but the row counts), rows every called sample is
    hom in (a = 2n: skipped), with and without missing calls, a haploid all-hom row, between ordinary rows"""
    rng = random.Random(9600)
    out = [vcfgen.header(ns)]
    pos = 100
    for k in range(30):
        kind = k % 6
        if kind == 0:
            gts = ["0|1"] * ns
        elif kind == 1:
            gts = ["1|1"] * ns
        elif kind == 2:
            gts = ["1|1"] * ns
            for s in rng.sample(range(ns), 3):
                gts[s] = ".|."
        elif kind == 3:
            gts = ["1"] * ns
        elif kind == 4:
            gts = ["0|1"] * ns
            gts[rng.randrange(ns)] = ".|."
        else:
            gts = [rng.choice(["0|0", "0|1", "1|1", ".|."]) for _ in range(ns)]
            gts[0] = "0|1"
        pos += 5
        out.append(pt.snp_line(pos, gts))
    return "".join(out).encode()


def singleton_hom_vcf(ns=40, n_lines=12):
    """one hom carrier among ns: |z| = sqrt(2 (n - 1)) > 2 for the carrier, so its q has three non-zero limbs"""
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        gts = ["0|0"] * ns
        gts[(7 * k) % ns] = "1|1"
        if k % 3 == 0:
            gts[(7 * k + 1) % ns] = ".|."
        out.append(pt.snp_line(100 + 5 * k, gts))
    return "".join(out).encode()


FLUSH_ROWS = 150000


def flush_pattern():
    """eight genotypes whose two most frequent classes have low limbs of large size: 150 000 identical rows then overflow an
    int32 sum of low-limb products -> (genotype list, |l0 l0'| of the pair of samples that overflows)"""
    best = None
    for n_het in range(0, 7):
        for n_hom in range(0, 7 - n_het):
            n_ref = 8 - n_het - n_hom
            a = n_het + 2 * n_hom
            if a == 0 or a == 16:
                continue
            l0 = {g: limbs(q_exact(8, a, g))[0] for g in range(3)}
            counts = {0: n_ref, 1: n_het, 2: n_hom}
            for g1 in range(3):
                for g2 in range(g1, 3):
                    if counts[g1] >= (2 if g1 == g2 else 1) and counts[g2] >= 1:
                        v = abs(l0[g1] * l0[g2])
                        if best is None or v > best[0]:
                            best = (v, n_het, n_hom)
    v, n_het, n_hom = best
    return ["0|1"] * n_het + ["1|1"] * n_hom + ["0|0"] * (8 - n_het - n_hom), v


def flush_vcf():
    gts, _ = flush_pattern()
    line = pt.snp_line(100, gts)
    return (vcfgen.header(8) + line * FLUSH_ROWS).encode()


def small_inputs():
    """every small input of the table cases: {name: bytes}"""
    d = {"edge%d" % ns: edge_vcf(ns) for ns in SAMPLE_EDGES}
    d.update({"tile%d" % n: pt.tile_vcf(n) for n in pt.TILE_ROWS})
    d.update({"fuzz%d" % s[0]: pt.fuzz_vcf(s[0]) for s in pt.FUZZ})
    d.update({"rare300": pt.rare_vcf(300), "limit": pt.short_list_limit_vcf(), "halfmissing": pt.half_missing_vcf(),
              "allmissing": all_missing_sample_vcf(), "monomorphic": monomorphic_vcf(), "singleton": singleton_hom_vcf()})
    return d
