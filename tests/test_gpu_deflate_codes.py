"""Step 4 of k_deflate (def_codes in bvcf_deflate.hip.h: rank sort, Moffat-Katajainen lengths, the length limiter, the
run-length coded header, the three sizes and the choice) through bvcf_bench_deflate_codes, on histograms no text is
known to give: trees that would be deeper than 15 (7 for the code-length code), one or no distance, every run-length
edge, exact ties between the block forms.  The references are tests/deflate_read.py's; test_deflate_read_cpu.py checks
without a GPU that every case here still has the edge it is named for.

Measured on an MI355X, the limiter (miniz's heuristic) costs at most 0.7843 % (2 bits in 255, an 11-symbol code-length
code of the clen_deep family) more than the package-merge optimum over all families below: 0.0757 % at worst on the 15-bit
trees (the chain of 23), 0.3279 % in the random family.  The tests allow twice the worst, or 1 % of the optimum where
that is larger."""
import random

import pytest

import deflate_craft as dc
import deflate_read as dr

pytestmark = pytest.mark.gpu

LIMITER_EXCESS = 0.007843  # worst (cost - optimum) / optimum measured over every family of this file; see the docstring
SUM_MAX = dr.PIECE + 1


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def case(name, ll, d=None, n=None, **edge):
    """ll / d: {symbol: frequency} (or lists); the end-of-block code is counted once unless ll says otherwise"""
    hll, hd = [0] * 286, [0] * 30
    for s, f in (ll.items() if isinstance(ll, dict) else enumerate(ll)):
        hll[s] = f
    for s, f in ((d or {}).items() if isinstance(d or {}, dict) else enumerate(d)):
        hd[s] = f
    hll[256] = hll[256] or 1
    assert sum(hll) <= SUM_MAX and sum(hd) <= dr.PIECE, name
    if n is None:  # the text these tokens would make, as far as a piece goes
        n = min(dr.PIECE, sum(hll[:256]) + sum(f * dc.LEN_BASE[s - 257] for s, f in enumerate(hll) if s > 256))
    return dict(name=name, hll=hll, hd=hd, n=n, **edge)


def fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def chain(k):
    """the k smallest frequencies whose only least-deep Huffman tree is a chain (depth k - 1): each one more than the sum
    of all but the two before it.  1 1 1 3 4 7 11 18 ... (Lucas numbers): 23 of them still sum to less than a piece"""
    w = [1, 1, 1]
    while len(w) < k:
        w.append(sum(w[:-1]) + 1)
    return w[:k]


def partial_ties(w):
    """how many sums of the k smallest counts, k >= 2, equal one of the counts after them"""
    w = sorted(w)
    return sum(1 for k in range(2, len(w)) if sum(w[:k]) in w[k:])


def _place(k, where, size, rng, keep=None):
    """k symbol numbers of an alphabet: low, high or mixed; `keep` is always one of them"""
    pool = [s for s in range(size) if s != keep]
    syms = {"low": pool[:k - (keep is not None)], "high": pool[len(pool) - k + (keep is not None):],
            "mixed": rng.sample(pool, k - (keep is not None))}[where]
    syms = list(syms) + ([keep] if keep is not None else [])
    rng.shuffle(syms)
    return syms


def cases_deep():
    """trees deeper than 15: Fibonacci and minimal-chain frequencies on either tree and doubled; and Fibonacci counts with
    one count moved by one, which moves or adds equalities between a count and a partial sum of the counts before it,
    the comparisons that tree building decides by (partial_ties counts them: the unperturbed Fibonacci counts have one,
    1 + 1 = 2; `perturbed` holds the sorted counts)"""
    rng, out = random.Random(41), []
    for seq_name, seq in (("fib", fib), ("chain", chain)):
        for k in range(17, 24):
            w = seq(k)
            if sum(w) > SUM_MAX:
                continue  # (23 Fibonacci numbers are more than a piece; the chain of 23 is not)
            for where in ("low", "high", "mixed"):
                for mul in (1, 2):
                    if mul * sum(w) > dr.PIECE:
                        continue
                    syms = _place(k, where, 286, rng, keep=256)
                    out.append(case("%s%d ll %s x%d" % (seq_name, k, where, mul), {s: mul * f for s, f in zip(syms, w)}, depth_ll=k - 1))
                    syms = _place(k, where, 30, rng)
                    out.append(case("%s%d d %s x%d" % (seq_name, k, where, mul), {256: 1, 257: mul * sum(w)},
                                    {s: mul * f for s, f in zip(syms, w)}, depth_d=k - 1))
    for k in (18, 21):  # one count changed by one, every count in turn
        w = fib(k)
        for j in range(k):
            for dlt in (-1, 1):
                if w[j] + dlt < 1:
                    continue
                v = w[:j] + [w[j] + dlt] + w[j + 1:]
                out.append(case("fib%d ll [%d]%+d" % (k, j, dlt), dict(zip(_place(k, "mixed", 286, rng, keep=256), v)), perturbed=sorted(v)))
                out.append(case("fib%d d [%d]%+d" % (k, j, dlt), {257: sum(v)}, dict(zip(_place(k, "mixed", 30, rng), v)), perturbed=sorted(v)))
    return out


def cases_flat():
    out = [case("all 286 and all 30", [200] * 286, [2000] * 30, all_used=True),
           case("all 286 and all 30, ones", [1] * 286, [1] * 30, all_used=True)]
    for k in (2, 4, 8, 16, 32, 64, 128, 256):
        out.append(case("flat %d literals" % k, {s: 16 for s in range(k - 1)}, flat=k))
    for k in (2, 3, 8, 14, 15):
        out.append(case("powers of two, %d" % k, {s: 1 << s for s in range(k)}))
    out.append(case("only the end-of-block code", {}, used_ll=1, used_d=0))
    out.append(case("one literal", {65: 9}, used_ll=2))
    out.append(case("literal 0 only", {0: 1}, used_ll=2))
    out.append(case("two literals", {65: 9, 255: 9}, used_ll=3))
    for s in (0, 1, 29):
        out.append(case("one distance, symbol %d" % s, {65: 300, 257: 50}, {s: 50}, used_d=1))
        out.append(case("one distance, symbol %d, once" % s, {65: 1, 285: 1}, {s: 1}, used_d=1))
    for pair in ((0, 1), (0, 29), (28, 29)):
        out.append(case("two distances %d %d" % pair, {65: 30, 260: 7}, {pair[0]: 3, pair[1]: 4}, used_d=2))
    out.append(case("three distances", {65: 30, 260: 7}, {3: 3, 4: 3, 17: 1}, used_d=3))
    out.append(case("no distance", {s: 5 + s for s in range(40)}, used_d=0))
    return out


def dyadic(lens):
    """frequencies 2^(15 - L): the only optimal code of a complete set of lengths is that set"""
    return {s: 1 << (15 - l) for s, l in enumerate(lens) if l}


def _interleave(counts):
    """a sequence with counts[v] times v and no value four times in a row"""
    left, seq = dict(counts), []
    while any(left.values()):
        v = max((v for v in left if left[v] and (len(seq) < 1 or seq[-1] != v)), key=lambda v: (left[v], v))
        seq.append(v)
        left[v] -= 1
    return seq


# lengths L with counts whose entries make the code-length histogram a chain: found by search over the permutations of
# lengths 2..11 for sum(count * 2^-L) == 1
CL_CHAIN = [((4, 7, 11, 18, 29, 47), (3, 8, 5, 11, 10, 9)), ((4, 7, 11, 18, 29, 47), (6, 4, 10, 11, 8, 7)),
            ((4, 7, 11, 18, 29, 47), (11, 4, 6, 8, 7, 9)), ((4, 7, 11, 18, 29, 47), (11, 6, 7, 5, 9, 8)),
            ((4, 7, 11, 18, 29, 47, 76), (5, 6, 8, 11, 10, 9, 7))]


def cases_clen_deep():
    """the 7-bit limit of the code-length code: forced lengths laid out so that the run-length entries are 1 x 16, 1 x 18,
    1 x `2`, 3 x 0 and 4, 7, 11, 18, 29, 47 (, 76) of six (seven) lengths: ten (eleven) code-length symbols in a chain"""
    out = []
    for counts, lens in CL_CHAIN:
        seq = _interleave(dict(zip(lens, counts)))
        zeros = 257 - len(seq) - 3  # one run for an 18, hlit = 257
        assert 11 <= zeros <= 138 and 2 not in lens
        lit = seq[:5] + [0] + seq[5:9] + [0, 0] + seq[9:20] + [0] * zeros + seq[20:]
        assert len(lit) == 257 and lit[256]
        # four distances of length 2: the entries `2`, then 16 for three more
        out.append(case("clen chain %s" % (lens,), dyadic(lit), {0: 5, 1: 5, 2: 5, 3: 5}, lit=lit, clen_syms=len(lens) + 4))
    return out


# the entries the rule makes of a run of zeros / of a run of lengths 7 (after another length)
ZERO_RUN_ENTRIES = {1: [(0, 0)], 2: [(0, 0)] * 2, 3: [(17, 0)], 10: [(17, 7)], 11: [(18, 0)], 12: [(18, 1)], 137: [(18, 126)],
                    138: [(18, 127)], 139: [(18, 127), (0, 0)], 140: [(18, 127), (0, 0), (0, 0)], 141: [(18, 127), (17, 0)],
                    148: [(18, 127), (17, 7)], 149: [(18, 127), (18, 0)], 150: [(18, 127), (18, 1)]}
ZERO_RUNS = tuple(ZERO_RUN_ENTRIES)
SEVENS_ENTRIES = {1: [(7, 0)], 2: [(7, 0)] * 2, 3: [(7, 0)] * 3, 4: [(7, 0), (16, 0)], 5: [(7, 0), (16, 1)], 6: [(7, 0), (16, 2)],
                  7: [(7, 0), (16, 3)], 8: [(7, 0), (16, 3), (7, 0)], 9: [(7, 0), (16, 3), (7, 0), (7, 0)],
                  10: [(7, 0), (16, 3), (16, 0)], 11: [(7, 0), (16, 3), (16, 1)]}


def rle_layouts():
    """-> (name, lit_lens, dist_lens): complete sets of lengths laid out for an edge of the run-length rule"""
    out = []
    for z in ZERO_RUNS:  # two lengths, z zeros, then a flat code's other lengths up to symbol 256
        lens = [l for l in dc.flat_lens(range(257 - z), 257 - z)]
        out.append(("zero run %d" % z, lens[:2] + [0] * z + lens[2:], [1, 1]))
    for r in range(1, 12):  # 8 8, r lengths 7, 8s: r * 2^-7 + (256 - 2r) * 2^-8 = 1; the last 8 is symbol 256
        out.append(("run of %d lengths 7" % r, [8, 8] + [7] * r + [8] * (253 - 2 * r) + [0] * (r + 1) + [8], [1, 1]))
    # a run that goes on from the last literal/length lengths into the distance lengths: 3 3 | 3 3 3 3 3 3 3 3
    out.append(("run across the boundary", [3] * 4 + [0] * 252 + [2] + [0] * 26 + [3, 3], [3] * 8))
    # hclen: a distance tree has at most 30 codes, so a length of 4 or less (or the two 1s of the two-code minimum) is
    # always sent and hclen is never below 12 (CLEN_ORDER[11] == 4); 19 needs a length 15
    out.append(("hclen 12: lengths 8 and 4", [8] * 100 + [0] * 13 + [8] * 156, [4] * 16))
    out.append(("hclen 19: a length 15", list(range(1, 16)) + [0] * 241 + [15], [1, 1]))
    return out


def cases_rle():
    out = []
    for name, lit, dist in rle_layouts():
        assert dr.kraft(lit) == 1 << 15 and dr.kraft(dist) == 1 << 15 and lit[256] and len(lit) <= 286, name
        out.append(case(name, dyadic(lit), dyadic(dist) if dist != [1, 1] else {}, lit=lit, dist=dist))
    return out


def cases_random(n_cases=300):
    rng, out = random.Random(77), []
    for i in range(n_cases):
        style = ("sparse", "dense", "skewed")[i % 3]
        if style == "sparse":
            ll = {rng.randrange(286): rng.randint(1, 400) for _ in range(rng.randint(1, 30))}
            d = {rng.randrange(30): rng.randint(1, 100) for _ in range(rng.randint(0, 5))}
        elif style == "dense":
            ll = {s: rng.randint(1, 200) for s in range(286) if rng.random() < 0.9}
            d = {s: rng.randint(1, 200) for s in range(30) if rng.random() < 0.9}
        else:
            base = rng.choice([1.3, 1.6, 2.0, 2.5])
            syms = rng.sample(range(286), rng.randint(5, 40))
            ll = {s: max(1, int(base ** min(j, 30))) for j, s in enumerate(syms)}
            d = {s: max(1, int(base ** j)) for j, s in enumerate(rng.sample(range(30), rng.randint(2, 24)))}
        ll[256] = ll.get(256) or 1
        for h, cap in ((ll, SUM_MAX), (d, dr.PIECE)):
            while sum(h.values()) > cap:
                for s in h:
                    h[s] = max(1, h[s] // 2)
        out.append(case("random %d %s" % (i, style), ll, d, n=rng.choice([None, rng.randint(0, dr.PIECE)])))
    return out


# (lengths of a dyadic shape -- the last one is the end-of-block code's --, first literal, scale) with fixed == dynamic in
# bytes: found by search over shapes and scales with dr.reference_sizes
FIX_DYN_TIES = [([1, 2, 3, 3], 0, 2), ([1, 3, 3, 3, 3], 144, 2)]
# histograms for the ties with the stored size: the first three code best dynamically, the last three fixed
STORED_TIES = [("flat 16", {s: 40 for s in range(15)}, {}), ("high literals", {s: 8 for s in range(192, 255)}, {}),
               ("matches", {65: 64, 66: 64, 257: 64, 256: 64}, {0: 32, 1: 32}),
               ("23 literals of 9 bits", {s: 1 for s in range(144, 167)}, {}), ("four of one literal", {0: 4}, {}),
               ("a short repeat", {65: 3, 66: 2, 258: 2}, {1: 2})]


def cases_ties():
    """exact ties of the byte sizes, each with its two neighbours, over histograms whose lengths are forced or whose fixed
    form is the smaller (so that the reference knows the sizes that tie): fixed == dynamic by the scale of a dyadic
    histogram, stored == fixed and stored == dynamic by the text length n, which only the stored size depends on"""
    out = []
    for lens, first, scale in FIX_DYN_TIES:
        for dt in (-1, 0, 1):
            ll = {first + i: (scale + dt) << (max(lens) - l) for i, l in enumerate(lens[:-1])}
            ll[256] = (scale + dt) << (max(lens) - lens[-1])
            out.append(case("fixed == dynamic: %s from %d x %d%+d" % (lens, first, scale, dt), ll, n=dr.PIECE,
                            tie=("fix", "dyn") if dt == 0 else None))
    for name, ll, d in STORED_TIES:
        c0 = case(name, ll, d, n=0)
        _, dyn_b, fix_b, _, _ = dr.reference_sizes(c0["hll"], c0["hd"], 0)
        which, b = ("dyn", dyn_b) if dyn_b < fix_b else ("fix", fix_b)  # the tie with the smaller of the two decides
        for dn in (-1, 0, 1):
            out.append(case("stored == %s: %s, n%+d" % (which, name, dn), ll, d, n=b - 5 + dn, tie=("sto", which) if dn == 0 else None))
    return out


FAMILIES = {"deep": cases_deep, "flat": cases_flat, "clen_deep": cases_clen_deep, "rle": cases_rle, "random": cases_random,
            "ties": cases_ties}


def check_case(c, lens, rle, out, excess):
    """every assertion of the issue on one case; excess collects (cost - optimum) / optimum of the limited trees"""
    name = c["name"]
    lit, dist, clen = [int(x) for x in lens[:286]], [int(x) for x in lens[286:316]], [int(x) for x in lens[316:]]
    kind, hdr, hlit, hdist, hclen, nr, dyn_b, fix_b = (int(x) for x in out)
    entries = [(int(e) & 0xFF, int(e) >> 8) for e in rle[:nr]]
    fcl = [0] * 19
    for s, _ in entries:
        fcl[s] += 1
    for what, freqs, got, limit in (("ll", c["hll"], lit, 15), ("d", c["hd"], dist, 15), ("cl", fcl, clen, 7)):
        got_cost = dr.check_lengths(freqs, got, limit, (name, what))
        want, depth = dr.huffman_cost(freqs)
        if sum(1 for f in freqs if f) < 2:
            continue
        if depth <= limit:
            assert got_cost == want, (name, what, got_cost, want)  # Moffat-Katajainen: optimal
        else:
            opt = dr.limited_cost(freqs, limit)
            excess.append(((got_cost - opt) / opt, name, what))
            assert opt <= got_cost <= opt + opt * max(2 * LIMITER_EXCESS, 0.01), (name, what, got_cost, opt, want)
    assert (hlit, hdist) == dr.trim(lit, dist), name
    assert hclen == dr.min_hclen(clen), name
    assert entries == dr.rle_rule(lit[:hlit] + dist[:hdist]), name
    assert hdr == dr.header_bits(hclen, clen, entries), name
    assert dyn_b == (hdr + dr.body_bits(c["hll"], c["hd"], lit, dist) + 7) >> 3, name
    assert fix_b == dr.fixed_bytes(c["hll"], c["hd"]), name
    assert kind == dr.choose(c["n"], dyn_b, fix_b)[0], (name, kind, c["n"] + 5, dyn_b, fix_b)
    # the edges that depend on what the device returned, asserted on it
    if "lit" in c:
        assert lit[:len(c["lit"])] == c["lit"] and not any(lit[len(c["lit"]):]), name
    if "dist" in c:
        assert dist[:len(c["dist"])] == c["dist"], name
    if "clen_syms" in c:
        assert sum(1 for f in fcl if f) == c["clen_syms"] and dr.huffman_cost(fcl)[1] > 7 and max(clen) == 7, (name, fcl)
    if c.get("tie"):
        sizes = {"sto": c["n"] + 5, "dyn": dyn_b, "fix": fix_b}
        assert sizes[c["tie"][0]] == sizes[c["tie"][1]], (name, sizes)
    if c.get("used_d") in (0, 1):
        assert sorted(l for l in dist if l) == [1, 1] and hdist == max(2, max(s for s, l in enumerate(dist) if l) + 1), name


def run_family(bv, cases):
    lens, rle, out = bv.bench_deflate_codes([(c["hll"], c["hd"], c["n"]) for c in cases])
    excess = []
    for i, c in enumerate(cases):
        check_case(c, lens[i], rle[i], out[i], excess)
    return excess, out


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_codes(bv, family):
    cases = FAMILIES[family]()
    excess, out = run_family(bv, cases)
    worst = max(excess, default=(0.0, "-", "-"))
    print("%s: %d cases, %d limited trees, worst excess over package-merge %.6f (%s %s)" % ((family, len(cases), len(excess)) + worst))
    kinds = {int(o[0]) for o in out}
    if family in ("random", "ties", "flat"):
        assert kinds >= {dr.STORED, dr.DYNAMIC} and (family == "random" or dr.FIXED in kinds)
    if family in ("deep", "clen_deep"):
        assert len(excess) >= len(cases) // 2  # the limiter ran

