"""Whole pieces through bvcf_bgzf_deflate_device, read back token by token (tests/deflate_read.py): every member must
inflate to its piece, hold exactly the tokens of the reference tokenizer (steps 1 and 2 of k_deflate's header comment,
done sequentially), be the smallest of the three block forms of those tokens, and, where dynamic, carry the header that
def_codes gives for the histogram of those tokens (test_gpu_deflate_codes.py's assertions on it).  The texts are built
for the edges of the match finder and the parallel parse; test_deflate_read_cpu.py checks without a GPU that each still
holds the token it was built for."""
import gzip
import os
import random
import struct
import zlib

import pytest

import deflate_craft as dc
import deflate_read as dr
import test_gpu_deflate_codes as codes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = dr.PIECE
FILL, WORD = b"ACGT", b"abcdefghijklmnopqrstuvwxyz0123456789"


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def golden_tsv():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.expected.tsv.gz"), "rb") as f:
        return f.read(1 << 20)


def members(out):
    """the (payload, crc, isize) of every member of a BGZF stream"""
    ms, pos = [], 0
    while pos < len(out):
        assert out[pos:pos + 16] == b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
        total = struct.unpack_from("<H", out, pos + 16)[0] + 1
        ms.append((out[pos + 18:pos + total - 8],) + struct.unpack_from("<II", out, pos + total - 8))
        pos += total
    assert pos == len(out)
    return ms


def pieces_of(text):
    return [text[i:i + PIECE] for i in range(0, len(text), PIECE)]


def check_texts(bv, texts, stats=None):
    """every assertion of this file on every piece of every text; one device call per text, one call of the code builder
    and one of each inflater for all of them.  stats collects the kinds and what the callers assert on"""
    outs, recs = [], []
    for text in texts:
        out = bv.bgzf_deflate_device(text, add_eof=False)
        outs.append(out)
        ms = members(out)
        ps = pieces_of(text)
        assert len(ms) == len(ps)
        for (pay, crc, isize), piece in zip(ms, ps):
            assert isize == len(piece) and crc == zlib.crc32(piece)
            assert zlib.decompress(pay, -15) == piece  # zlib is the judge
            blocks, bits = dr.read_blocks(pay)
            assert len(blocks) == 1 and blocks[0]["bfinal"] == 1 and (bits + 7) >> 3 == len(pay)
            assert dr.expand(blocks) == piece
            recs.append((piece, blocks[0]))
    whole, stream = b"".join(texts), b"".join(outs)
    if stream:
        rc, got, _ = bv.bgzf_inflate_device(stream, cap=len(whole) + 64)
        assert rc == 0 and got == whole  # this repo's inflater
        rc, got, _ = bv.decompress(stream)
        assert rc == 0 and got == whole  # the driver's host reader
    want = [dr.tokenize(piece) for piece, _ in recs]
    hists = [dr.histograms(t) for t in want]
    lens, rle, out = bv.bench_deflate_codes([(hll, hd, len(piece)) for (hll, hd), (piece, _) in zip(hists, recs)])
    for i, ((piece, blk), toks) in enumerate(zip(recs, want)):
        where = (i, len(piece), piece[:24])
        kind, size = dr.choose(len(piece), int(out[i][6]), int(out[i][7]))
        assert blk["btype"] == kind and (blk["bits"] + 7) >> 3 == size, where
        # (whatever form wins: the sizes that decide, and the dynamic lengths behind dyn_b, against the references)
        codes.check_case(dict(name=str(where), hll=hists[i][0], hd=hists[i][1], n=len(piece)), lens[i], rle[i], out[i], [])
        if kind != dr.STORED:
            assert blk["tokens"] == toks, where
        if kind == dr.DYNAMIC:
            hlit, hdist, hclen, nr = (int(x) for x in out[i][2:6])
            assert (blk["hlit"], blk["hdist"], blk["hclen"]) == (hlit, hdist, hclen), where
            assert blk["lit_lens"] == [int(x) for x in lens[i][:hlit]] and blk["dist_lens"] == [int(x) for x in lens[i][286:286 + hdist]], where
            assert blk["clen_lens"] == [int(x) for x in lens[i][316:]], where
            assert blk["rle"] == [(int(e) & 0xFF, int(e) >> 8) for e in rle[i][:nr]], where
        if stats is not None:
            stats.append(dict(kind=kind, tokens=toks, block=blk, n=len(piece)))
    return recs


# ---- the texts

def _fill(rng, n):
    return bytes(rng.choice(FILL) for _ in range(n))


def _word(rng, n):
    return bytes(rng.choice(WORD) for _ in range(n))


def token_at(tokens, pos):
    """the token of a parse that starts at text position pos, or None"""
    x = 0
    for t in tokens:
        if x == pos:
            return t
        x += 1 if isinstance(t, int) else t[0]
    return None


SENTINELS = [v for v in range(1, 256) if v not in FILL + WORD + b"\n"]


def match_unit(rng, length, a, b, end="mismatch", source_len=None, k=0):
    """a text that starts on a chunk boundary: a line end, a bytes of filler, a word of source_len letters, filler up to b bytes past
    the next chunk boundary, the first `length` letters of the word again, then another letter than the source's next
    (or nothing: the end of the piece).  The byte before the match is SENTINELS[k], which a piece holds once, so that no
    match from before can run into it.  -> (text, position of the match, its distance); the reference tokenizer must
    find (length, distance) there, else other letters are tried"""
    source_len = source_len or length + 1
    for _ in range(50):
        s = _word(rng, source_len)
        head = b"\n" + _fill(rng, a) + s  # (the line end: whatever stands before the unit, the match cannot start early)
        head += _fill(rng, -len(head) % 256 + b)
        head = head[:-1] + bytes([SENTINELS[k % len(SENTINELS)]])
        p = len(head)
        if end == "cap":
            tail = s + _fill(rng, 3)
            length = min(258, source_len)
        else:
            tail = s[:length] + (bytes([rng.choice([c for c in WORD if c != s[length]])]) + _fill(rng, 3) if end == "mismatch" else b"")
        text = head + tail
        if token_at(dr.tokenize(text), p) == (length, p - a - 1):
            return text, p, p - a - 1
    raise AssertionError("no unit for %r" % ((length, a, b, end),))


def pack(units):
    """units, each from a chunk boundary on and none across a piece boundary -> (text, [(position, token)])"""
    text, wants = bytearray(), []
    for u, p, d, length in units:
        text += b"A" * (-len(text) % 256)
        if len(text) % PIECE + len(u) > PIECE:
            text += b"A" * (-len(text) % PIECE)
        wants.append((len(text) + p, (length, d)))
        text += u
    return bytes(text), wants


def texts_lengths():
    """every match length 4..258 ended by a mismatch (packed into a few pieces) and by the end of the piece (a text each),
    the 258 cap with longer sources; the source and the match at all alignments mod 4"""
    rng = random.Random(5)
    units = []
    for length in range(4, 259):
        k = length * 7 + 3
        u, p, d = match_unit(rng, length, k & 3, (k >> 2) & 3, k=len(units))
        units.append((u, p, d, length))
    for a in range(4):
        for b in range(4):
            for src in (258, 259, 261, 300 + a):
                u, p, d = match_unit(rng, 258, a, b, "cap", src, k=len(units))
                units.append((u, p, d, 258))
            u, p, d = match_unit(rng, 7 + a + 4 * b, a, b, k=len(units))
            units.append((u, p, d, 7 + a + 4 * b))
    packed = pack(units)
    ends = []
    for length in range(4, 259):
        k = length * 5 + 1
        u, p, d = match_unit(rng, length, k & 3, (k >> 2) & 3, "end")
        ends.append((u, [(p, (length, d))]))
    return [packed] + ends


def dist_text(rng, dist, length=9):
    """one piece: a word, filler, the word again `dist` after it, then a mismatch.  Distances up to 256 as a period of
    `dist` letters that starts `dist` before the first chunk boundary"""
    for _ in range(200):
        if dist <= 256:
            per = _word(rng, dist)
            head = _fill(rng, 256 - dist)
            text = head + (per * (length + dist))[:dist + length] + _fill(rng, 4)
            p = 256
        else:
            s = _word(rng, length + 1)
            a = rng.randrange(4)
            head = _fill(rng, a) + s
            head += _fill(rng, dist - len(s))
            p = len(head)
            text = head + s[:length] + bytes([rng.choice([c for c in WORD if c != s[length]])]) + _fill(rng, 40)
        toks = dr.tokenize(text)
        got = token_at(toks, p)
        if dist <= dr.MAX_DIST and got == (length, dist) and p >= 256:
            return text, [(p, got)]
        # (too far: a literal BECAUSE of the distance -- the table entry p looks at is the word, equal on its 4 bytes)
        if dist > dr.MAX_DIST and got == text[p] and dr.candidate(text, p) == p - dist and text[p - dist:p - dist + 4] == text[p:p + 4]:
            return text, [(p, got)]
    raise AssertionError("no text for distance %d" % dist)


DISTS = sorted(set([1, 2, 3, 4] + [d for s in range(30) for d in (dc.DIST_BASE[s], (dc.DIST_BASE[s + 1] if s < 29 else 32769) - 1)] +
                   [32767, 32768, 32769]))


def texts_distances():
    rng = random.Random(6)
    out = [dist_text(rng, d) for d in DISTS]
    # a 4-gram whose latest earlier occurrence is in the SAME chunk: the match goes to the one in an earlier chunk
    for _ in range(50):
        s = _word(rng, 12)
        text = _fill(rng, 100) + s + b"!" + _fill(rng, 256 - 113 + 20) + s + b"?" + _fill(rng, 30) + s + b"#" + _fill(rng, 10)
        p1, p2 = 276, 276 + 13 + 30
        toks = dr.tokenize(text)
        if p2 < 512 and token_at(toks, p1) == (12, p1 - 100) and token_at(toks, p2) == (12, p2 - 100):
            out.append((text, [(p1, (12, p1 - 100)), (p2, (12, p2 - 100))]))
            break
    else:
        raise AssertionError("no same-chunk text")
    return out


def text_single_distance():
    rng = random.Random(7)
    blockk = bytes(rng.randrange(256) for _ in range(300))
    return blockk * 60


def texts_sweep(source):
    src = {"golden": golden_tsv, "two_letter": lambda: bytes(random.Random(8).choice(b"ab") for _ in range(2 * PIECE)),
           "period7": lambda: b"GATTACA" * (2 * PIECE // 7 + 1)}[source]()
    return [src[:n] for n in list(range(0, 601)) + list(range(65270, 65291))]


def texts_stored_fixed_tie():
    return [bytes(range(144, 144 + k)) for k in range(21, 32)]


def texts_rle_layouts():
    """the run-length layouts of test_gpu_deflate_codes.py that a literal-only text of at most 256 bytes can carry as a
    dynamic block: the zero runs from 137 on, whose 120 or fewer used literals of lengths 6 and 7 fit once (127 bytes) and
    twice (254).  -> (zero run, text, the laid-out lengths).  The others cannot be written so: zero runs up to 12 and the
    runs of lengths 7 need some 250 literals of length 8, one byte each, which stored beats; the run across the boundary
    and the hclen 12 layout need distances, which a text without an earlier chunk has none of"""
    rng, out = random.Random(12), []
    for name, lit, _ in codes.rle_layouts():
        z = int(name.split()[-1]) if name.startswith("zero run") else 0
        if z < 137:
            continue
        for scale in (1, 2):
            t = [s for s, l in enumerate(lit[:256]) if l for _ in range(scale << (7 - l))]
            rng.shuffle(t)
            out.append((z, bytes(t), lit))
    return out


def texts_fixed_matches():
    """a first chunk of 256 bytes below 144 (eight bits each under the fixed code, too flat to pay for a dynamic header;
    no matches: it has no earlier chunk), then 8 to 200 bytes of it again: short texts whose matches a fixed block carries"""
    rng, out = random.Random(9), []
    for x in list(range(8, 40)) + list(range(40, 201, 7)):
        first = bytes(rng.randrange(144) for _ in range(256))
        q = rng.randrange(0, 257 - x)
        out.append(first + first[q:q + x] + (first[5:5 + x // 3] if x % 2 else b""))
    return out


def texts_segments():
    """258-byte matches that jump over many of the ceil(n / 256)-byte segments of the parallel parse, and a match that ends
    on a segment end and one byte to either side"""
    rng, out = random.Random(10), []
    for n in (260, 300, 511, 512, 513, 777, 1024, 2000, 3333, 5000):
        per = _word(rng, rng.choice([1, 3, 17, 64]))
        out.append((_fill(rng, 256 - len(per)) + per * n)[:n])
    for n in (1025, 2049, 4097):  # seg = 5, 9, 17
        seg = (n + 255) // 256
        for off in (-1, 0, 1):
            for _ in range(50):
                s = _word(rng, 8)
                end = seg * (256 // seg + 9) + off  # a segment end past the first chunk, give or take one
                head = _fill(rng, 3) + s + b"."
                head += _fill(rng, end - 8 - len(head))
                text = head + s + b"!" + _fill(rng, n - len(head) - 9)
                if len(text) == n and token_at(dr.tokenize(text), end - 8) == (8, end - 8 - 3):
                    out.append(text)
                    break
            else:
                raise AssertionError("no segment text")
    return out


def texts_random(n_texts=200):
    out = []
    for seed in range(n_texts):
        rng = random.Random(1000 + seed)
        alphabet = b"01|/.\t\n:,ACGT" * 6 + bytes(rng.randrange(256) for _ in range(rng.choice([0, 4, 40])))
        target = rng.choice([rng.randint(1, 300), rng.randint(300, 3000), 5000]) if seed % 25 else rng.choice([20000, PIECE])
        if seed % 10 == 3:  # (bytes that do not compress: stored)
            out.append(bytes(rng.randrange(256) for _ in range(target)))
            continue
        tokens, pos = [], 0
        while pos < target:
            if pos == 0 or rng.random() < 0.35:
                t = bytes(rng.choice(alphabet) for _ in range(min(rng.choice([1, 1, 2, 5, 19]), target - pos)))
                tokens.append(t)
                pos += len(t)
                continue
            dist = rng.choice([1, 2, 3, 4, 8, rng.choice(dc.EDGE_DISTS), rng.randint(1, 32768)])
            length = min(rng.choice(dc.EDGE_LENS + [rng.randint(3, 258), 258]), target - pos)
            if length >= 3:
                tokens.append((length, min(dist, pos)))
                pos += length
        out.append(bytes(dc.expand(tokens)))
    return out


LARGE_GRID = 512


def large_text():
    """1 029 pieces and 7 bytes: a cycle of 37 kinds of piece -- dynamic (TSV, letters), stored (random bytes), fixed-size
    candidates (short periods compress to almost nothing) -- so that every workgroup of the grid takes a second and a
    third piece, some straight after a stored one, and the call is split after 1 028 pieces"""
    rng = random.Random(11)
    tsv = golden_tsv()
    cycle = []
    for k in range(37):
        if k % 3 == 0:
            cycle.append(tsv[k * 1000:k * 1000 + PIECE])
        elif k % 3 == 1:
            cycle.append(bytes(rng.getrandbits(8) for _ in range(PIECE)))
        else:
            cycle.append((_word(rng, 1 + k) * PIECE)[:PIECE] if k % 2 else bytes(rng.choice(b"ACGTN") for _ in range(PIECE)))
    text = b"".join(cycle[i % 37] for i in range(1029)) + b"\tthe end"[:7]
    return cycle, text


# ---- the tests

def _check_wants(texts_wants, stats):
    i = 0
    for text, wants in texts_wants:
        for piece_no in range(len(pieces_of(text))):
            st = stats[i]
            i += 1
            for pos, tok in wants:
                if pos // PIECE == piece_no:
                    assert st["kind"] != dr.STORED and token_at(st["tokens"], pos % PIECE) == tok, (pos, tok)


@pytest.mark.parametrize("source", ["golden", "two_letter", "period7"])
def test_length_sweep(bv, source):
    texts = texts_sweep(source)
    assert bv.bgzf_deflate_device(texts[0], add_eof=False) == b""
    stats = []
    check_texts(bv, texts[1:], stats)
    assert {s["n"] for s in stats} >= set(range(1, 601)) | {PIECE, 1, 10}


def test_forced_match_lengths(bv):
    tw = texts_lengths()
    stats = []
    check_texts(bv, [t for t, _ in tw], stats)
    _check_wants(tw, stats)


def test_forced_distances(bv):
    tw = texts_distances()
    stats = []
    check_texts(bv, [t for t, _ in tw], stats)
    _check_wants(tw, stats)


def test_single_distance(bv):
    stats = []
    check_texts(bv, [text_single_distance()], stats)
    blk = stats[0]["block"]
    assert stats[0]["kind"] == dr.DYNAMIC and {t[1] for t in stats[0]["tokens"] if not isinstance(t, int)} == {300}
    ds = dc.match_syms(4, 300)[2]
    assert blk["hdist"] == ds + 1 and [s for s, l in enumerate(blk["dist_lens"]) if l] == [0, ds]  # def_huff_lengths, m == 1
    assert blk["dist_lens"][0] == blk["dist_lens"][ds] == 1


def test_stored_fixed_tie(bv):
    stats = []
    check_texts(bv, texts_stored_fixed_tie(), stats)
    assert {s["kind"] for s in stats} == {dr.STORED, dr.FIXED}
    assert all(isinstance(t, int) for s in stats for t in s["tokens"])


def test_rle_layouts_as_texts(bv):
    layouts = texts_rle_layouts()
    stats = []
    check_texts(bv, [t for _, t, _ in layouts], stats)
    for (z, text, lit), st in zip(layouts, stats):
        want = codes.ZERO_RUN_ENTRIES[z]
        assert st["kind"] == dr.DYNAMIC and st["block"]["lit_lens"] == lit, (z, len(text))
        assert st["block"]["rle"][2:2 + len(want) + 1] == want + [(lit[2 + z], 0)], (z, len(text))  # as the member sends them


def test_fixed_blocks_with_matches(bv):
    stats = []
    check_texts(bv, texts_fixed_matches(), stats)
    fixed = [s for s in stats if s["kind"] == dr.FIXED]
    assert len(fixed) >= 10 and all(any(not isinstance(t, int) for t in s["tokens"]) for s in fixed)


def test_segment_edges(bv):
    stats = []
    check_texts(bv, texts_segments(), stats)
    assert sum(1 for s in stats for t in s["tokens"] if not isinstance(t, int) and t[0] == 258) >= 30


def test_random_pieces(bv):
    stats = []
    check_texts(bv, texts_random(), stats)
    assert {s["kind"] for s in stats} == {dr.STORED, dr.FIXED, dr.DYNAMIC}


def test_large_call(bv):
    cycle, text = large_text()
    out = bv.bgzf_deflate_device(text, add_eof=False)
    assert gzip.decompress(out) == text
    ms = members(out)
    assert len(ms) == 1030 and ms[-1][2] == 7
    alone = [members(bv.bgzf_deflate_device(p, add_eof=False))[0] for p in cycle]
    kinds = [(m[0][0] >> 1) & 3 for m in alone]
    assert set(kinds) >= {dr.STORED, dr.DYNAMIC}
    # a workgroup's next piece is a grid further on: 512 on an MI355X (256 CUs x 2), and (i + 512) % 37 == (i + 31) % 37,
    # so pieces coded after a stored one (the `continue` of the loop over pieces) are those of kind k with k - 31 stored
    assert LARGE_GRID % 37 == 31 and 2 * LARGE_GRID < 1029 < 3 * LARGE_GRID
    after_stored = {kinds[(k + 31) % 37] for k in range(37) if kinds[k] == dr.STORED}
    assert after_stored >= {dr.STORED, dr.DYNAMIC}
    for k in range(37):
        occ = [i for i in range(1029) if i % 37 == k]
        for i in (occ[0], occ[1], occ[-1]):
            assert ms[i] == alone[k], (k, i)
