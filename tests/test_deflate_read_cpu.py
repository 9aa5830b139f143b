"""tests/deflate_read.py against deflate_craft.py and zlib, and the inputs of test_gpu_deflate_codes.py and
test_gpu_deflate_tokens.py against the references (no GPU): the reader returns what the writer wrote, the reference
tokenizer's tokens mean the text, package-merge is no worse than a clipped Huffman code, and every crafted histogram and
text still has the edge it is named for.  So a device test that fails there fails for the compressor's sake."""
import random
import zlib

import pytest

import deflate_craft as dc
import deflate_read as dr
import test_gpu_deflate_codes as codes
import test_gpu_deflate_tokens as toks
import test_gpu_inflate_craft as craft


def flat(tokens):
    """deflate_craft tokens as the reader returns them: literal bytes one by one, matches as (length, distance)"""
    out = []
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, bytes):
            out += list(t)
        else:
            ls, lx, ds, dx = dc.raw_of(t)
            out.append((dc.LEN_BASE[ls - 257] + lx, dc.DIST_BASE[ds] + dx))
    return out


def test_reader_returns_what_the_writer_wrote():
    rng = random.Random(21)
    for seed in range(60):
        text = bytes(rng.choice(b"ACGT\t\n01") for _ in range(rng.choice([1, 7, 300, 5000])))
        tokens = dc.tokenize(text, rng)
        lit, dist = dc.random_lens(tokens, rng)
        blocks = [dc.fixed(tokens, False), dc.stored(text[:100], False), dc.dynamic(tokens, lit, dist, True)]
        recs, bits = dr.read_blocks(dc.payload(*blocks))
        assert [r["btype"] for r in recs] == [dr.FIXED, dr.STORED, dr.DYNAMIC] and [r["bfinal"] for r in recs] == [0, 0, 1]
        assert recs[0]["tokens"] == flat(tokens) == recs[2]["tokens"] and bytes(recs[1]["tokens"]) == text[:100]
        assert recs[2]["lit_lens"] == lit and recs[2]["dist_lens"] == dist
        assert (recs[2]["hlit"], recs[2]["hdist"], recs[2]["hclen"]) == (len(lit), len(dist), 19)
        assert recs[2]["rle"] == dc._rle(lit + dist)
        assert dr.expand(recs) == text + text[:100] + text
        assert sum(r["bits"] for r in recs) == bits and (bits + 7) >> 3 == len(dc.payload(*blocks))
    # the writer's edges: the crafted members of the inflater's tests that carry their tokens and lengths
    n = 0
    for c in craft.cases_b() + craft.cases_a(0):
        if "tokens" not in c or any(not isinstance(t, (int, bytes)) and t[0] in ("raw", "bits") for t in c["tokens"]):
            continue
        recs, _ = dr.read_blocks(c["member"][18:-8])
        assert dr.expand(recs) == c["text"], c["name"]
        if len(recs) == 1:
            assert recs[0]["tokens"] == flat(c["tokens"]), c["name"]
            if "lit_lens" in c and recs[0]["btype"] == dr.DYNAMIC:
                assert recs[0]["lit_lens"] == list(c["lit_lens"]) and recs[0]["dist_lens"] == list(c["dist_lens"]), c["name"]
            n += 1
    assert n >= 40


def test_reader_against_zlib():
    rng = random.Random(22)
    texts = [b"", b"a", b"GATTACA" * 999, bytes(rng.choice(b"ACGT\t\n.|01") for _ in range(70000)),
             bytes(rng.getrandbits(8) for _ in range(3000)), toks.golden_tsv()[:200000]]
    for text in texts:
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                                (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY)):
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
            pay = c.compress(text) + c.flush()
            recs, bits = dr.read_blocks(pay)
            assert dr.expand(recs) == text == zlib.decompress(pay, -15) and (bits + 7) >> 3 == len(pay)
            if strategy == zlib.Z_FIXED:
                assert dr.DYNAMIC not in {r["btype"] for r in recs}
            if strategy == zlib.Z_HUFFMAN_ONLY:
                assert all(isinstance(t, int) for r in recs for t in r["tokens"])


def test_package_merge_and_huffman():
    rng = random.Random(23)
    seen_limited = 0
    for i in range(120):
        k = rng.randint(2, 40)
        base = rng.choice([1.0, 1.3, 1.7, 2.2])
        freqs = [0] * 60
        for j, s in enumerate(rng.sample(range(60), k)):
            freqs[s] = max(1, int(base ** (j % 24) * rng.uniform(1, 2)))
        want, depth = dr.huffman_cost(freqs)
        for limit in (15, 7, 6):
            if k > 1 << limit:
                continue
            pm = dr.package_merge(freqs, limit)
            lens = [pm.get(s, 0) for s in range(60)]
            assert max(lens) <= limit and dr.kraft(lens, limit) == 1 << limit
            got = dr.cost(freqs, lens)
            if depth <= limit:
                assert got == want
            else:
                seen_limited += 1
                # a Huffman code with its depths clipped to the limit is not a code any more; the heuristic repair of
                # the device (tested on the GPU) is one, and package-merge is no worse than any
                assert got > want
                clipped = sorted(min(d, limit) for d in dr.huffman_depths(freqs).values())
                while sum(1 << (limit - l) for l in clipped) > 1 << limit:  # push the deepest short code down
                    j = max(j for j, l in enumerate(clipped) if l < limit)
                    clipped[j] += 1
                by_freq = sorted((f for f in freqs if f), reverse=True)
                assert got <= sum(f * l for f, l in zip(by_freq, clipped))
    assert seen_limited >= 20
    assert dr.huffman_depths([0, 5, 0]) == {1: 1} and dr.huffman_cost([1, 1, 2, 3, 5, 8]) == (1 * 5 + 1 * 5 + 2 * 4 + 3 * 3 + 5 * 2 + 8, 5)


def test_rle_rule_and_sizes():
    assert dr.rle_rule([0] * 139) == [(18, 127), (0, 0)] and dr.rle_rule([0] * 149) == [(18, 127), (18, 0)]
    assert dr.rle_rule([0] * 141) == [(18, 127), (17, 0)] and dr.rle_rule([0] * 10 + [3]) == [(17, 7), (3, 0)]
    assert dr.rle_rule([5] * 7) == [(5, 0), (16, 3)] and dr.rle_rule([5] * 8) == [(5, 0), (16, 3), (5, 0)]
    assert dr.rle_rule([5] * 10) == [(5, 0), (16, 3), (16, 0)] and dr.rle_rule([5] * 3 + [0, 0]) == [(5, 0)] * 3 + [(0, 0)] * 2
    rng = random.Random(24)
    for _ in range(200):  # the entries mean the sequence
        seq = []
        while len(seq) < 316:
            seq += [rng.choice([0, 0, rng.randint(1, 15)])] * rng.choice([1, 1, 2, 3, 4, 7, 11, 12, 140])
        seq = seq[:316]
        back = []
        for s, x in dr.rle_rule(seq):
            back += [back[-1]] * (3 + x) if s == 16 else [0] * (3 + x) if s == 17 else [0] * (11 + x) if s == 18 else [s]
        assert back == seq
    assert dr.choose(23, 30, 28) == (dr.STORED, 28) and dr.choose(24, 30, 28) == (dr.FIXED, 28)
    assert dr.choose(25, 30, 30) == (dr.STORED, 30) and dr.choose(26, 30, 30) == (dr.FIXED, 30) and dr.choose(26, 30, 31) == (dr.DYNAMIC, 30)


# ---- the inputs of test_gpu_deflate_codes.py

def test_code_cases_hold_their_edges():
    n_deep = 0
    for family, make in codes.FAMILIES.items():
        cases = make()
        assert len({c["name"] for c in cases}) == len(cases)
        for c in cases:
            assert sum(c["hll"]) <= dr.PIECE + 1 and sum(c["hd"]) <= dr.PIECE and c["hll"][256] >= 1 and 0 <= c["n"] <= dr.PIECE, c["name"]
            (cl, dl), (cd, dd) = dr.huffman_cost(c["hll"]), dr.huffman_cost(c["hd"])
            if "depth_ll" in c:
                assert dl == c["depth_ll"] >= 16, c["name"]
            if "depth_d" in c:
                assert dd == c["depth_d"] >= 16, c["name"]
            n_deep += dl > 15 or dd > 15
            if "used_d" in c:
                assert sum(1 for f in c["hd"] if f) == c["used_d"], c["name"]
            if "used_ll" in c:
                assert sum(1 for f in c["hll"] if f) == c["used_ll"], c["name"]
            if c.get("all_used"):
                assert all(c["hll"]) and all(c["hd"])
            if "lit" in c:  # forced lengths: the Huffman depths are the layout, and no other code costs as little
                d = dr.huffman_depths(c["hll"])
                assert [d.get(s, 0) for s in range(len(c["lit"]))] == c["lit"], c["name"]
                assert all(f == 1 << (15 - c["lit"][s]) for s, f in enumerate(c["hll"]) if f), c["name"]
            if "clen_syms" in c:
                fcl = [0] * 19
                for s, _ in dr.rle_rule(c["lit"] + [2, 2, 2, 2]):
                    fcl[s] += 1
                assert sum(1 for f in fcl if f) == c["clen_syms"] >= 9 and dr.huffman_cost(fcl)[1] > 7, c["name"]
                assert sorted(f for f in fcl if f)[:4] == [1, 1, 1, 3]
            if c.get("tie"):
                _, dyn_b, fix_b, _, _ = dr.reference_sizes(c["hll"], c["hd"], c["n"])
                sizes = {"sto": c["n"] + 5, "dyn": dyn_b, "fix": fix_b}
                assert sizes[c["tie"][0]] == sizes[c["tie"][1]] == min(sizes.values()), c["name"]
    assert n_deep >= 200
    ties = [c["tie"] for c in codes.cases_ties() if c.get("tie")]
    assert {("sto", "fix"), ("sto", "dyn"), ("fix", "dyn")} <= set(ties)
    # the perturbed Fibonacci counts: still skewed trees, and a count more makes every later partial sum equal a count,
    # where the unperturbed counts have the one equality 1 + 1 = 2
    perturbed = [c["perturbed"] for c in codes.cases_deep() if "perturbed" in c]
    assert len(perturbed) == 148 and codes.partial_ties(codes.fib(18)) == codes.partial_ties(codes.fib(21)) == 1
    assert {min(codes.partial_ties(w), 3) for w in perturbed} == {1, 2, 3}
    assert sum(1 for w in perturbed if codes.partial_ties(w) > 1) >= 60
    assert all(dr.huffman_cost([0] + w)[1] >= 9 for w in perturbed)


def test_run_length_layouts():
    """every layout yields the entries it is named for, by the reference rule, where the layout puts them"""
    by = {name: (lit, dist, dr.rle_rule(lit + dist)) for name, lit, dist in codes.rle_layouts()}
    assert len(by) == len(codes.ZERO_RUNS) + 11 + 3
    for z, want in codes.ZERO_RUN_ENTRIES.items():
        lit, _, got = by["zero run %d" % z]
        assert lit[2:2 + z] == [0] * z and lit[1] and lit[2 + z]
        assert got[2:2 + len(want) + 1] == want + [(lit[2 + z], 0)], z
    for r, want in codes.SEVENS_ENTRIES.items():
        lit, _, got = by["run of %d lengths 7" % r]
        assert lit[:2 + r + 1] == [8, 8] + [7] * r + [8]
        assert got[:2 + len(want) + 1] == [(8, 0), (8, 0)] + want + [(8, 0)], r
    lit, dist, got = by["run across the boundary"]
    assert lit[-2:] == [3, 3] and dist == [3] * 8 and got[-3:] == [(3, 0), (16, 3), (16, 0)]
    for name, hclen in (("hclen 12: lengths 8 and 4", 12), ("hclen 19: a length 15", 19)):
        assert dr.min_hclen([sum(1 for s, _ in by[name][2] if s == v) for v in range(19)]) == hclen
    # as texts: literal-only, dynamic by the reference, the laid-out lengths forced, the entries as named
    layouts = toks.texts_rle_layouts()
    assert sorted({z for z, _, _ in layouts}) == [137, 138, 139, 140, 141, 148, 149, 150] and len(layouts) == 16
    assert sorted({len(t) for _, t, _ in layouts})[-1] <= 256
    for z, text, lit in layouts:
        parsed = dr.tokenize(text)
        assert all(isinstance(x, int) for x in parsed)
        hll, hd = dr.histograms(parsed)
        d = dr.huffman_depths(hll)
        assert [d.get(s, 0) for s in range(257)] == lit, (z, len(text))
        kind, dyn_b, fix_b, _, _ = dr.reference_sizes(hll, hd, len(text))
        assert kind == dr.DYNAMIC and dyn_b < min(fix_b, len(text) + 5), (z, len(text), dyn_b, fix_b)
        want = codes.ZERO_RUN_ENTRIES[z]
        assert dr.rle_rule(lit + [1, 1])[2:2 + len(want)] == want


# ---- the inputs of test_gpu_deflate_tokens.py

def _expands(text):
    for i in range(0, len(text), dr.PIECE):
        piece = text[i:i + dr.PIECE]
        t = dr.tokenize(piece)
        assert bytes(dc.expand(t)) == piece
        assert all(isinstance(x, int) or (4 <= x[0] <= 258 and 1 <= x[1] <= 32768) for x in t)
    return True


def _wants_hold(texts_wants):
    for text, wants in texts_wants:
        _expands(text)
        parsed = {i: dr.tokenize(text[i * dr.PIECE:(i + 1) * dr.PIECE]) for i in {p // dr.PIECE for p, _ in wants}}
        for pos, tok in wants:
            assert toks.token_at(parsed[pos // dr.PIECE], pos % dr.PIECE) == tok, (pos, tok)
            hll, hd = dr.histograms(parsed[pos // dr.PIECE])
            n = len(text[pos // dr.PIECE * dr.PIECE:][:dr.PIECE])
            assert min(dr.fixed_bytes(hll, hd), n + 5) < n + 5, "a stored block would hide the tokens"


def test_match_length_texts():
    tw = toks.texts_lengths()
    _wants_hold(tw)
    packed = tw[0][1]
    assert {t[0] for _, t in packed} == set(range(4, 259))
    assert {(pos % 4, (pos - t[1]) % 4) for pos, t in packed} == {(p, q) for p in range(4) for q in range(4)}
    assert {(pos % 4, (pos - t[1]) % 4) for pos, t in packed if t[0] == 258} == {(p, q) for p in range(4) for q in range(4)}
    ends = tw[1:]
    assert [w[0][1][0] for _, w in ends] == list(range(4, 259))
    assert all(w[0][0] + w[0][1][0] == len(text) for text, w in ends)  # the match ends the piece
    # the mismatch at each byte of the last word of the word-wise extension, for each alignment of the match
    assert {((t[0] - 4) % 4, pos % 4) for pos, t in packed} == {(r, p) for r in range(4) for p in range(4)}


def test_distance_texts():
    tw = toks.texts_distances()
    _wants_hold(tw)
    got = {t[1] for _, w in tw for _, t in w if not isinstance(t, int)}
    assert got >= {d for d in toks.DISTS if d <= 32768} and max(got) == 32768
    assert {dc.match_syms(4, d)[2] for d in got} == set(range(30))
    # the word 32 769 back must stay literals, and for the distance's sake: it IS the table entry, equal on its 4 bytes
    far = [(text, w[0][0]) for text, w in tw if isinstance(w[0][1], int)]
    assert len(far) == 1
    text, p = far[0]
    assert dr.candidate(text, p) == p - 32769 and text[p - 32769:p - 32765] == text[p:p + 4]
    near = [(text, w[0][0]) for text, w in tw if w[0][1] == (9, 32768)]
    assert len(near) == 1 and dr.candidate(near[0][0], near[0][1]) == near[0][1] - 32768


def test_other_texts():
    for source in ("golden", "two_letter", "period7"):
        texts = toks.texts_sweep(source)
        assert [len(t) for t in texts] == list(range(601)) + list(range(65270, 65291))
        for t in texts[:601:7] + texts[601::5]:
            _expands(t)
    t = toks.text_single_distance()
    parsed = dr.tokenize(t)
    assert _expands(t) and {x[1] for x in parsed if not isinstance(x, int)} == {300}
    assert sum(1 for f in dr.histograms(parsed)[1] if f) == 1
    kinds = set()
    for t in toks.texts_stored_fixed_tie():
        parsed = dr.tokenize(t)
        assert len(t) <= 256 and all(isinstance(x, int) for x in parsed)
        hll, hd = dr.histograms(parsed)
        fix_b = dr.fixed_bytes(hll, hd)
        assert fix_b == (8 * len(t) + len(t) + 10 + 7) >> 3
        kinds.add((fix_b <= len(t) + 4, fix_b == len(t) + 5))
    assert kinds == {(True, False), (False, True), (False, False)}  # fixed wins, the tie, stored wins
    with_matches = 0
    for t in toks.texts_fixed_matches():
        parsed = dr.tokenize(t)
        assert _expands(t) and 264 <= len(t) <= 256 + 200 + 70
        hll, hd = dr.histograms(parsed)
        with_matches += any(not isinstance(x, int) for x in parsed) and dr.fixed_bytes(hll, hd) < len(t) + 5
    assert with_matches >= 30
    segs = toks.texts_segments()
    assert all(_expands(t) for t in segs) and min(len(t) for t in segs) == 260 and max(len(t) for t in segs) == 5000
    assert sum(1 for t in segs for x in dr.tokenize(t) if not isinstance(x, int) and x[0] == 258) >= 30
    for t in toks.texts_random()[::4]:
        _expands(t)
