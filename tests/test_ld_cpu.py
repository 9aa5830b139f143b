"""--ld / --ldPrune, the host half: the exported pair counts and predicate against the reference of ldpairs.py, the
--ldR2 text rules, the seam state machine fed batches cut anywhere, the layout of bvcf_config_ld, and the conditions the
inputs of test_gpu_ld.py must meet (with the oracle alone).  No device."""
import ctypes as C
import random

import numpy as np
import pytest

import ldpairs as lp
import oracle_lib as orc
import pairtable as pt


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def random_hom(rng, n, S, miss=0.1):
    cls = rng.choice(4, size=(n, S), p=[0.5, 0.2, 0.3 - miss, miss])
    return (cls == 1).astype(np.uint8), (cls == 2).astype(np.uint8), (cls == 3).astype(np.uint8)


def ref_counts(H, O, M, a, b):
    G, V = lp.genotypes(H, O, M)
    return lp.six_counts(G[a], V[a], G[b], V[b])


# ---- the counts

@pytest.mark.parametrize("S", list(range(1, 71)) + [127, 128, 129, 2504])
def test_counts_match_reference(bv, S):
    rng = np.random.default_rng(100 + S)
    H, O, M = random_hom(rng, 6, S)
    bed = lp.bed_rows(H, O, M)
    for a in range(5):
        for b in range(a + 1, 6):
            assert bv.ld_counts(bed[a].tobytes(), bed[b].tobytes(), S) == ref_counts(H, O, M, a, b), (S, a, b)


def test_all_class_pairs_in_every_position_of_a_byte(bv):
    """9 samples: position p of the first two bytes holds each of the 16 (class a, class b) pairs, the others are missing
    in row a, so that the counts are those of the one sample"""
    g = {0: 0, 1: 1, 2: 2}
    for p in range(8):
        for ca in range(4):
            for cb in range(4):
                cls = np.full((2, 9), 3, dtype=np.int64)
                cls[1, :] = 1
                cls[0, p], cls[1, p] = ca, cb
                H, O, M = ((cls == q).astype(np.uint8) for q in (1, 2, 3))
                bed = lp.bed_rows(H, O, M)
                got = bv.ld_counts(bed[0].tobytes(), bed[1].tobytes(), 9)
                want = [0] * 6 if 3 in (ca, cb) else [1, g[ca], g[cb], g[ca] ** 2, g[cb] ** 2, g[ca] * g[cb]]
                assert got == want == ref_counts(H, O, M, 0, 1), (p, ca, cb)


@pytest.mark.parametrize("S", [1, 2, 3, 5, 6, 7, 17, 66])
def test_pad_bits_are_ignored(bv, S):
    rng = np.random.default_rng(300 + S)
    H, O, M = random_hom(rng, 2, S)
    bed = lp.bed_rows(H, O, M)
    want = bv.ld_counts(bed[0].tobytes(), bed[1].tobytes(), S)
    keep = (1 << (2 * (S % 4))) - 1 if S % 4 else 0xFF
    for fill_a, fill_b in ((0xFF, 0xFF), (0xAA, 0x00), (0x00, 0xAA), (0x55, 0xFF)):
        a, b = bed[0].copy(), bed[1].copy()
        a[-1] = (a[-1] & keep) | (fill_a & ~keep & 0xFF)
        b[-1] = (b[-1] & keep) | (fill_b & ~keep & 0xFF)
        assert bv.ld_counts(a.tobytes(), b.tobytes(), S) == want == ref_counts(H, O, M, 0, 1)


# ---- the predicate

T6S = [0, 1, 333333, 333334, 10 ** 6]


def triples():
    out = [[4, 2, 1, 2, 1, 1],           # the example: c = 2, va = 4, vb = 3
           [4, 0, 2, 0, 2, 0],           # va = 0
           [4, 2, 0, 2, 0, 0],           # vb = 0
           [4, 4, 4, 4, 4, 4],           # both 0
           [4, 2, 2, 2, 2, 0],           # c < 0: c = -4, va = vb = 4 -> r2 = 1
           [6, 3, 4, 3, 6, 1],           # c < 0, r2 < 1
           [0, 0, 0, 0, 0, 0], [1, 1, 2, 1, 4, 2]]
    big = (1 << 24) - 1                  # counts near 2^24: c^2 * 10^6 passes 2^64 by far
    h = big // 2
    out += [[big, h, h, h, h, h],                       # a = b, all het or ref: r2 = 1
            [big, h, h, h, h, h - 1],
            [big, h, h + 1, h, h + 1, h],
            [big, 2 * h, 2 * h, 4 * h, 4 * h, 4 * h],   # hom or ref
            [big, 2 * h, h, 4 * h, h, 0]]               # never together: c < 0
    rng = random.Random(5)
    for _ in range(200):
        n = rng.choice([7, 100, 2504, big])
        ga = [rng.choice([0, 1, 2]) for _ in range(min(n, 64))]
        gb = [rng.choice([0, 1, 2]) if rng.random() < 0.5 else x for x in ga]
        scale = n // len(ga)
        out.append([scale * len(ga), scale * sum(ga), scale * sum(gb), scale * sum(x * x for x in ga),
                    scale * sum(x * x for x in gb), scale * sum(x * y for x, y in zip(ga, gb))])
    return out


def test_predicate_matches_python_integers(bv):
    seen = set()
    for k in triples():
        for t6 in T6S:
            want = lp.in_ld(k, t6)
            assert bv.ld_in_ld(k, t6) == want, (k, t6)
            seen.add(want)
        c, va, vb = lp.moments(k)
        if c * c * 10 ** 6 >= 1 << 64:
            seen.add("wide")
    assert seen == {True, False, "wide"}
    assert bv.ld_in_ld([4, 2, 1, 2, 1, 1], 333333) and not bv.ld_in_ld([4, 2, 1, 2, 1, 1], 333334)
    assert not bv.ld_in_ld([4, 0, 2, 0, 2, 0], 0) and not bv.ld_in_ld([4, 2, 0, 2, 0, 0], 0)
    assert bv.ld_in_ld([4, 2, 2, 2, 2, 0], 10 ** 6)
    with pytest.raises(ValueError):
        bv.ld_in_ld([1 << 24, 0, 0, 0, 0, 0], 0)
    with pytest.raises(ValueError):
        bv.ld_in_ld([4, 2, 1, 2, 1, 1], 10 ** 6 + 1)


# ---- --ldR2

def test_ld_r2_text_rules(bv):
    good = {"0": 0, "1": 10 ** 6, "0.2": 200000, "0.333333": 333333, "0.000001": 1, "1.0": 10 ** 6, "1.000000": 10 ** 6,
            "0.0": 0, "0.5": 500000, "0.25": 250000, "0.999999": 999999}
    for text, t6 in good.items():
        assert bv.parse_ld_r2(text) == t6, text
    for text in ["", " 0.2", "0.2 ", "+0.2", "-0", ".2", "0.", "1.", "1.1", "1.000001", "2", "0.2e0", "2e-1", "0.3333333", "1.0000000",
                 "0,2", "0x1", "00.2", "01", "0.2\n", "1.0 ", "nan", "0..2"]:
        with pytest.raises(ValueError):
            bv.parse_ld_r2(text)


# ---- the seam

@pytest.fixture(scope="module")
def seam_case():
    """a few hundred rows with LD, chrom changes and missing calls, made without a VCF: H / O / M and the rows' columns"""
    rng = np.random.default_rng(77)
    n, S = 260, 37
    cls = np.zeros((n, S), dtype=np.int64)
    cur = rng.choice(3, size=S, p=[0.6, 0.25, 0.15])
    for r in range(n):
        u = rng.random()
        if u < 0.15:
            cur = rng.choice(3, size=S, p=[0.6, 0.25, 0.15])
        elif u < 0.3:
            cur = 2 - cur
        else:
            flip = rng.random(S) < 0.1
            cur = np.where(flip, rng.choice(3, size=S), cur)
        cls[r] = np.where(rng.random(S) < 0.05, 3, cur)
    H, O, M = ((cls == q).astype(np.uint8) for q in (1, 2, 3))
    rows = [(b"chr1" if r < 100 else b"chr2" if r < 180 else b"chrUn_KI270302v1", b"%d" % (100 + 7 * r), b"A", b"G") for r in range(n)]
    return H, O, M, rows


def whole_run(case, window, t6):
    H, O, M, rows = case
    ev = lp.events_of(H, O, M, [r[0] for r in rows], window, t6)
    kept = lp.prune(ev, len(rows))
    return ev, lp.table_text(ev, rows)[len(lp.HEADER):], lp.lists_text(kept, rows)


def through_seam(bv, case, window, t6, cuts, ev):
    H, O, M, rows = case
    bed, loci = lp.bed_rows(H, O, M), lp.loci_of(rows)
    seam = bv.LdSeam(H.shape[1], window, t6)
    edges = [0] + list(cuts) + [len(rows)]
    for lo, hi in zip(edges, edges[1:]):
        seam.push(bed[lo:hi], lp.batch_events(ev, lo, hi), loci[lo:hi])
    got = seam.read(0), (seam.read(1), seam.read(2)), seam.counts()
    seam.close()
    return got


@pytest.mark.parametrize("window,t6", [(5, 200000), (50, 200000), (3, 0), (512, 10 ** 6)])
def test_seam_seeded_cuts(bv, seam_case, window, t6):
    ev, table, lists = whole_run(seam_case, window, t6)
    n = len(seam_case[3])
    assert 0 < len(ev)
    rng = random.Random(window)
    plans = [[], [n // 2], sorted(rng.sample(range(1, n), 12)),
             # batches of 0, 1 and fewer than `window` rows in a row: the carry spans three batches and more
             [40, 40, 41, 42, 42, 44, 45, 47, 48, 100, 100, 101, 179, 180, 181, 259],
             list(range(1, n))]
    for cuts in plans:
        got_table, got_lists, (n_rows, n_pairs) = through_seam(bv, seam_case, window, t6, cuts, ev)
        assert got_table == table, cuts
        assert got_lists == lists, cuts
        assert (n_rows, n_pairs) == (n, len(ev))


def test_seam_every_cut_position(bv, seam_case):
    """the first 40 rows, window 4: one cut at every position, and two cuts at every pair of positions up to 12"""
    H, O, M, rows = seam_case
    small = (H[:40], O[:40], M[:40], rows[:40])
    ev, table, lists = whole_run(small, 4, 100000)
    assert len(ev) > 5 and lists[1]
    for cut in range(0, 41):
        assert through_seam(bv, small, 4, 100000, [cut], ev)[:2] == (table, lists), cut
    for c1 in range(0, 13):
        for c2 in range(c1, 13):
            assert through_seam(bv, small, 4, 100000, [c1, c2], ev)[:2] == (table, lists), (c1, c2)


def test_seam_refuses_contradictions(bv, seam_case):
    H, O, M, rows = seam_case
    bed, loci = lp.bed_rows(H, O, M), lp.loci_of(rows)
    for bad in ([[5, 6, 1, 0, 0, 0, 0, 0]],                                  # d > b
                [[50, 1, 1, 0, 0, 0, 0, 0]],                                 # no such row
                [[5, 1, 1, 0, 0, 0, 0, 0], [5, 2, 1, 0, 0, 0, 0, 0]],        # a descending
                [[6, 1, 1, 0, 0, 0, 0, 0], [5, 1, 1, 0, 0, 0, 0, 0]]):       # b descending
        seam = bv.LdSeam(H.shape[1], 4, 0)
        with pytest.raises(ValueError):
            seam.push(bed[:10], np.array(bad, dtype=np.uint32), loci[:10])
        seam.close()
    with pytest.raises(ValueError):
        bv.LdSeam(10, 0, 0)
    with pytest.raises(ValueError):
        bv.LdSeam(10, 513, 0)
    with pytest.raises(ValueError):
        bv.LdSeam(1 << 24, 50, 0)


# ---- the config

def test_config_ld_layout_and_defaults(bv):
    L, T, M_ = bv.ConfigLd, bv.ConfigTrios, bv.ConfigMore
    assert L.trios.offset == 0 and L.ld_path.offset == C.sizeof(T) and C.sizeof(L) == C.sizeof(T) + 32
    assert bv.CONFIG_MORE_LD == 4
    c = L()
    C.memset(C.byref(c), 0xA5, C.sizeof(c))
    bv.lib.bvcf_config_ld_defaults(C.byref(c))
    assert c.trios.more.base.reserved[0] == bv.CONFIG_MORE and c.trios.more.base.reserved[1] == 4
    assert (c.ld_path, c.ld_prune_prefix, c.ld_window, c.ld_t6, c.ld_t6_set) == (None, None, 50, 200000, 1)
    assert c.trios.fam_path is None and c.trios.mendel_path is None
    # the older defaults write what they wrote: the new bytes stay as they were
    for fn, size, marker in (("bvcf_config_trios_defaults", C.sizeof(T), 3), ("bvcf_config_plink_defaults", C.sizeof(M_), 2),
                             ("bvcf_config_gate_defaults", C.sizeof(M_), 1), ("bvcf_config_more_defaults", C.sizeof(M_), 0)):
        c = L()
        C.memset(C.byref(c), 0xA5, C.sizeof(c))
        getattr(bv.lib, fn)(C.byref(c))
        raw = C.string_at(C.byref(c), C.sizeof(c))
        assert raw[size:] == b"\xA5" * (C.sizeof(c) - size), fn
        assert c.trios.more.base.reserved[1] == marker, fn


# ---- the inputs of the GPU tests

@pytest.mark.parametrize("name", ["ld40", "ld129", "ld300"])
def test_gpu_inputs_meet_their_conditions(name):
    vcf, window = lp.seeded_inputs()[name]
    assert b"\n1\t" in vcf and b"\nchr1\t" in vcf
    seen = set()
    for t6 in (200000, 10 ** 6):
        want, _, _ = lp.expected(orc.run, vcf, window, t6)
        seen |= lp.coverage(want, window)
        assert want["prune_out"] and want["prune_in"]
    assert seen >= lp.NEEDED, lp.NEEDED - seen
    # raw "1" and "chr1" are one chromosome: a pair in LD across the change
    want, _, _ = lp.expected(orc.run, vcf, window, 200000)
    raw = [ln.split(b"\t")[0] for ln in vcf.split(b"\n") if ln and not ln.startswith(b"#")]
    assert raw.count(b"1") and all(r[0] != b"1" for r in want["rows"])


def test_example_of_the_definitions():
    vcf = lp.exact_third_vcf()
    at, _, _ = lp.expected(orc.run, vcf, 50, 333333)
    above, _, _ = lp.expected(orc.run, vcf, 50, 333334)
    assert at["events"].tolist() == [[1, 1, 4, 2, 1, 2, 1, 1]] and len(above["events"]) == 0
    assert at["table"] == lp.HEADER + b"chr7\t100\tA\tG\t200\tA\tG\t4\t0.333\t+\n"
    assert at["prune_in"] == b"chr7:100:A:G\n" and at["prune_out"] == b"chr7:200:A:G\n"
    assert above["prune_in"] == b"chr7:100:A:G\nchr7:200:A:G\n" and above["prune_out"] == b""
