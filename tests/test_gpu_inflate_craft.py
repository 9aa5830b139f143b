"""k_inflate / k_inflate_w16 / k_inflate_w4 / k_crc32 over DEFLATE streams that zlib's compressor never writes: built
symbol by symbol with deflate_craft (match placement, code shapes, block mixes, member sizes), written by libdeflate
(tests/golden/libdeflate_*), and malformed in one stated way each.  The oracle is zlib's inflater
(test_deflate_craft_cpu.py holds every case of this module against it, without a GPU); here the device must give the
same bytes, or refuse.

Why every refused member ENDS on the device (k_inflate_body, bvcf_inflate.hip.h; the host then sees a status != 0 or a
CRC that differs and answers E_FATAL):

  R1   block type 3                          type == 3 -> kInfBadBlockType
  R2   NLEN is not ~LEN                      (len ^ nlen) != 0xFFFF -> kInfBadStored
  R3   stored LEN past the payload           q + len > in_len -> kInfInputOverrun, before a byte is copied
  R4   stored LEN past ISIZE                 pos + len > isize -> kInfOutputOverrun, before a byte is copied
  R5   HLIT field 30, 31                     n_lit > 286 -> kInfBadCodeLengths
  R6   HDIST field 30, 31                    n_dist > 30 -> kInfBadCodeLengths
  R7   over-subscribed code-length, literal  inf_build returns false before it fills a table -> kInfBadCodeLengths
       or distance code
  R8   code 16 as the first length           got == 0 -> kInfBadCodeLengths
  R9   a repeat past HLIT + HDIST            got + rep > want -> kInfBadCodeLengths, before lens[] is written
  R10  no end-of-block code (also: HCLEN     lit_lens[256] == 0 -> kInfBadCodeLengths
       field 0, which can send no length)
  R11  fixed-code symbols 286, 287           sym > 285 -> kInfBadSymbol
  R12  fixed distance symbols 30, 31         dsym > 29 -> kInfBadDistance
  R13  distance past the start of the text   dist > pos -> kInfBadDistance
  R14  the unused code of a 1-code distance  the table entry is 0, slow_decode finds no code in 15 steps and gives
       tree                                  0xFFFF: dsym > 29 -> kInfBadDistance
  R15  literal / match past ISIZE; stream    pos >= isize, pos + len > isize -> kInfOutputOverrun, both before the
       short of ISIZE                        write; pos != isize at the end -> kInfSizeMismatch
  R16  payload cut inside a symbol           fetch() zero-fills past in_len.  Every symbol takes >= 1 bit, so in_pos
                                             grows until refill() sees in_pos > in_len + 16 -> kInfInputOverrun, unless
                                             the zeros end the stream first (fixed code: 0000000 is end-of-block; a
                                             following block header 000 is a stored block with LEN = NLEN = 0 ->
                                             kInfBadStored) or the text reaches ISIZE -> kInfOutputOverrun; text that
                                             ends at ISIZE by chance is left to the CRC
  R17  right text, wrong CRC                 the host's compare of k_crc32's value with the trailer

Every one of these checks sits in front of the write it guards: no case makes the kernel write or read out of bounds.

Left different from the plan: "HCLEN = 4" as a VALID block does not exist -- with four code-length codes (16, 17, 18, 0)
no length but 0 can be sent, so there is no end-of-block code; it is refuse case R10b here, and the smallest valid
count, five (16, 17, 18, 0, 8), is the valid case hclen5."""
import functools
import os
import random
import struct
import subprocess
import zlib

import pytest

import deflate_craft as dc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


@pytest.fixture(autouse=True, params=["w32", "w16", "w4"])
def window(request, monkeypatch):
    """the three inflate kernels: the 32 KiB window, and the 16 and 4 KiB ones that read older bytes back from memory"""
    monkeypatch.setenv("BVCF_INFLATE_W16", {"w32": "0", "w16": "1", "w4": "2"}[request.param])
    return request.param


# ------------------------------------------------------------------ the cases (no GPU needed to build them)
# a case: {"name", "member", "text"} and, where a property of it is asserted, "tokens" / "want" / "lit_lens" / "dist_lens"

@functools.lru_cache(None)
def _base():
    """40 000 bytes of noise below 144 (8-bit fixed codes): no two places alike, so a copy from the wrong place shows"""
    rng = random.Random(950)
    return bytes(rng.randrange(144) for _ in range(40000))


def lits(n, at=0):
    b = _base()
    return (b[at:] + b * 2)[:n]


def case(name, *blocks, text, tail=b"", **more):
    return dict(name=name, member=dc.member(dc.payload(*blocks, tail=tail), bytes(text)), text=bytes(text), **more)


def fixed_case(name, tokens, **more):
    return case(name, dc.fixed(tokens, True), text=dc.expand(tokens), tokens=tokens, **more)


def flat(tokens, full=False):
    """(lit_lens, dist_lens) of flat complete codes over what the tokens use, or over all 286 + 30 symbols"""
    if full:
        return dc.flat_lens(range(286), 286), dc.flat_lens(range(30), 30)
    lit, dist = dc.symbols(tokens)
    lit = lit | ({0} if len(lit) < 2 else set())
    return dc.flat_lens(lit, max(257, max(lit) + 1)), (dc.flat_lens(dist, max(dist) + 1) if dist else [0])


def dyn_case(name, tokens, lens=None, **kw):
    lens = lens or flat(tokens)
    return case(name, dc.dynamic(tokens, lens[0], lens[1], True, **kw), text=dc.expand(tokens), tokens=tokens,
                lit_lens=lens[0], dist_lens=lens[1])


A_LENS = (3, 4, 5, 63, 64, 65, 66, 257, 258)
A_WINDOWS = (4096, 16384, 32768)
A_OVERLAP_DISTS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 257)


@functools.lru_cache(None)
def cases_a(W):
    """A. match placement around a window of W bytes (its segments are W / 2); W = 0: matches that overlap themselves"""
    out = []

    def add(kind, pos, length, dist):
        tokens = [lits(pos), (length, dist)]
        if pos + 2 * length + 258 <= dc.MAX_MEMBER:  # the same match again, behind a run that fills a copy's every lane
            tokens += [(258, 1), (length, dist)]
        out.append(fixed_case("%s W=%d pos=%d len=%d dist=%d" % (kind, W, pos, length, dist), tokens, want=[(pos & 3, length, dist)],
                              kind=kind, W=W))

    if W == 0:
        for dist in A_OVERLAP_DISTS:
            for length in sorted({max(3, dist + 1), 64, 65, 258}):
                tokens, pos, want = [lits(300)], 300, []
                for a in (1, 2, 3, 0):  # the match at every alignment of its first byte
                    n = (a - pos - 1) % 4 + 1
                    tokens += [lits(n, pos), (length, dist)]
                    want.append((a, length, dist))
                    pos += n + length
                out.append(fixed_case("overlap len=%d dist=%d" % (length, dist), tokens, want=want, kind="overlap", W=0))
        return out
    for length in A_LENS:
        for a in range(4):
            for kind, dist in [("sum%+d" % d, W + d - length) for d in (-1, 0, 1)] + [("dist%+d" % d, W + d) for d in (-1, 0, 1)]:
                if dist <= 32768:
                    add(kind, dist + ((a - dist) & 3), length, dist)
    # the ring's oldest byte inside one lane's four-byte group
    for s in range(1, 6):
        for length in (4, 65, 258):
            for a in range(4):
                dist = W - length + s
                if dist <= 32768:
                    add("oldest+%d" % s, dist + ((a - dist) & 3), length, dist)
    # a far match that starts at a segment flush, and ones that cross it
    for k in (2, 3):
        p = k * W // 2
        if p + 258 <= dc.MAX_MEMBER:
            for length in (9, 258):
                add("seg_at", p, length, W - 7)
            add("seg_cross", p - 100, 258, min(W - 7, p - 101))
            add("seg_cross", p - 2, 5, W - 3)
            add("seg_cross", p - 1, 66, W - 60)
    if W == 32768:
        for a in (0, 1, 2, 3, 4, 5, 258, 1000, 32768 - 258):
            for length in (3, 258):
                add("dist32768", 32768 + a, length, 32768)
    return out


def _vcf_text():
    import vcfgen
    return vcfgen.gen_vcf(77, 120, 150, weird=0.02)


@functools.lru_cache(None)
def cases_b():
    """B. codes"""
    out = []
    rng = random.Random(1951)
    # fifteen literals + end-of-block with lengths 1, 2, .., 14, 15, 15: the 15-bit codes go through the canonical walk
    alphabet = b"ACGT01|/\t\n.:,;="
    text = alphabet + bytes(rng.choice(alphabet) for _ in range(400))
    for v in range(6):
        lens = list(range(1, 15)) + [15, 15]
        if v >= 2:
            rng.shuffle(lens)
        syms = ([256] + list(alphabet)) if v == 0 else (list(alphabet) + [256])  # v 0: end-of-block is the 1-bit code, v 1: a 15-bit one
        lit_lens = [0] * 257
        for s, l in zip(syms, lens):
            lit_lens[s] = l
        out.append(dyn_case("lit15 v%d" % v, [text], (lit_lens, [0])))
    for v in range(4):
        dist_lens = list(range(1, 15)) + [15, 15]
        rng.shuffle(dist_lens)
        tokens = [lits(300)]
        for ds in list(range(16)) * 3:
            tokens.append((rng.randint(3, 12), dc.DIST_BASE[ds] + rng.randrange(1 << dc.DIST_EXTRA[ds])))
            tokens.append(rng.randrange(144))
        out.append(dyn_case("dist15 v%d" % v, tokens, (flat(tokens)[0], dist_lens)))
    # HLIT = 286, HDIST = 30, HCLEN = 19: every length symbol at its smallest and largest extra bits (284 + 31 is 258)
    tokens = [lits(700)]
    for ls in range(257, 286):
        for lx in (0, (1 << dc.LEN_EXTRA[ls - 257]) - 1):
            ds = rng.randrange(18)
            tokens += [("raw", ls, lx, ds, rng.randrange(1 << dc.DIST_EXTRA[ds])), rng.randrange(144)]
    assert ("raw", 284, 31) in [t[:3] for t in tokens if isinstance(t, tuple)]
    out.append(dyn_case("all length symbols", tokens, flat(tokens, True)))
    # every distance symbol at its smallest and largest extra bits
    tokens = [lits(32768)]
    for ds in range(30):
        for dx in (0, (1 << dc.DIST_EXTRA[ds]) - 1):
            tokens += [(rng.choice([3, 4, 11, 258]), dc.DIST_BASE[ds] + dx), rng.randrange(144)]
    out.append(dyn_case("all distance symbols", tokens, flat(tokens, True)))
    # how the code lengths are sent
    vcf = _vcf_text()
    tokens = dc.tokenize(vcf[3000:9000], rng)
    out.append(dyn_case("no repeat codes", tokens, rle=False))
    out.append(dyn_case("flat codes, repeat codes", tokens))
    lit_lens = [0] * 259  # A, C, end-of-block: 2 bits; lengths 3 and 4: 3 bits, like the first two of the five distance codes
    for s, l in ((65, 2), (67, 2), (256, 2), (257, 3), (258, 3)):
        lit_lens[s] = l
    tokens = [b"ACCA", (3, 1), (4, 2), b"C", (3, 3), (4, 4), (3, 5), b"AC", (4, 6)]
    out.append(dyn_case("16 across the literal/distance boundary, maximal 18", tokens, (lit_lens, [3, 3, 2, 2, 2]),
                        rle=[(18, 54), (2, 0), (0, 0), (2, 0), (18, 127), (18, 39), (2, 0), (3, 0), (16, 0), (2, 0), (2, 0), (2, 0)]))
    lit_lens = [0] * 257
    for s in (65, 67, 71, 256):
        lit_lens[s] = 2
    out.append(dyn_case("16 after 18", [b"GACAGGCA" * 9], (lit_lens, [0]),
                        rle=[(18, 40), (16, 0), (16, 3), (17, 2), (2, 0), (0, 0), (2, 0), (17, 0), (2, 0), (18, 127), (16, 3), (18, 29),
                             (2, 0), (0, 0)]))
    out.append(dyn_case("hclen5", [bytes(rng.randrange(255) for _ in range(500))], ([8] * 255 + [0, 8], [0]), hclen=5))
    out.append(dyn_case("one distance code: symbol 0", [b"abc", (200, 1), b"x", (3, 1)], (flat([b"abcx", (200, 1), (3, 1)])[0], [1])))
    tokens = [b"abcde", (200, 4), b"x", (3, 4)]
    out.append(dyn_case("one distance code: symbol 3", tokens, (flat(tokens)[0], [0, 0, 0, 1])))
    out.append(dyn_case("HDIST = 1 with length 0", [b"only literals here\n" * 20]))
    only_eob = ([0] * 256 + [1], [0])
    out.append(case("empty dynamic block alone", dc.dynamic([], *only_eob, True), text=b""))
    out.append(case("empty dynamic blocks, then text", dc.dynamic([], *only_eob, False), dc.dynamic([], *only_eob, False),
                    dc.fixed([b"after nothing"], True), text=b"after nothing"))
    for seed in range(64):
        r = random.Random(seed)
        n = r.choice([50, 700, 5000, 20000])
        at = r.randrange(len(vcf) - n)
        tokens = dc.tokenize(vcf[at:at + n], r, r.choice([4, 300, 32768]))
        out.append(dyn_case("random_code seed %d" % seed, tokens, dc.random_lens(tokens, r)))
    return out


def _to_size(size, near_end_dist, kind):
    """tokens of exactly `size` bytes of text: noise, long distance-1 runs, and a last match `near_end_dist` back"""
    tokens, pos = [lits(33000)], 33000
    while size - pos > 258 + 200:
        tokens += [(258, 1), lits(1, pos)[0]]
        pos += 259
    tokens.append(lits(size - pos - 200, pos))
    tokens.append((200, near_end_dist))
    assert len(dc.expand(tokens)) == size
    return dyn_case("isize %d dynamic" % size, tokens) if kind == "dynamic" else fixed_case("isize %d fixed" % size, tokens)


@functools.lru_cache(None)
def cases_c():
    """C. blocks and sizes"""
    out = []
    rng = random.Random(1952)
    for k in range(9):  # 9-bit literals: the stored block's LEN field at every bit alignment
        head = bytes(rng.randrange(144, 256) for _ in range(k))
        out.append(case("stored after %d fixed literals" % k, dc.fixed([head] if k else [], False), dc.stored(lits(100 + k), True),
                        text=head + lits(100 + k)))
    out.append(case("empty stored blocks", dc.stored(b"", False), dc.fixed([b"abc"], False), dc.stored(b"", False),
                    dc.stored(b"def", False), dc.stored(b"", True), text=b"abcdef"))
    out.append(case("one empty stored block", dc.stored(b"", True), text=b""))
    text = bytearray(lits(100))
    blocks = [dc.fixed([lits(100)], False), dc.stored(lits(40000, 100), False)]
    text += lits(40000, 100)
    tokens = [(258, 20000), (258, 32768), (100, 4097), (3, 16385), (258, 1)]
    blocks.append(dc.fixed(tokens, True))
    out.append(case("stored block across segments, matched into", *blocks, text=dc.expand(tokens, text)))
    out.append(case("stored block of 65500", dc.stored(lits(65500), True), text=lits(65500)))
    chars = rng.choices(b"ACGT\n", k=1000)
    out.append(case("1000 dynamic blocks of one literal", *[dc.dynamic([b], *flat([b]), i == 999) for i, b in enumerate(chars)],
                    text=bytes(chars)))
    # every block copies from the ones before it
    text, blocks = bytearray(), []
    parts = [[lits(5000)], [(258, 5000), (100, 4096), 7, (258, 4097)], [(30, 5500), (258, 1), (4, 4095)], [(258, 2), (258, 5000), 9],
             [(65, 6000), (3, 6200)]]
    for i, part in enumerate(parts):
        at = len(text)
        dc.expand(part, text)
        last = i == len(parts) - 1
        blocks.append([dc.fixed(part, last), dc.dynamic(part, *flat(part), last), dc.stored(text[at:], last)][i % 3])
    out.append(case("blocks that match into the blocks before", *blocks, text=text))
    out.append(case("final empty fixed block", dc.fixed([b"hello"], False), dc.fixed([], True), text=b"hello"))
    out.append(case("empty fixed block alone", dc.fixed([], True), text=b""))
    out.append(case("garbage after the final block", dc.fixed([b"hello, hello", (20, 7)], True), tail=b"\xff\x00\xaa\x55\x07" * 5,
                    text=dc.expand([b"hello, hello", (20, 7)])))
    for size in (65535, 65536):
        out.append(_to_size(size, 32768, "fixed"))
        out.append(_to_size(size, 32768, "dynamic"))
        out.append(_to_size(size, 3, "fixed"))
    return out


SWEEP_SIZES = (list(range(0, 1101)) + [2047, 2048, 2049, 16383, 16384, 16385, 32767, 32768, 32769, 65279, 65280, 65281] +
               list(range(65500, 65506)))


@functools.lru_cache(None)
def cases_sweep():
    """stored members of every size k_crc32's start value and the write-out's tail can meet (65 505: the most a member holds stored)"""
    rng = random.Random(1953)
    noise = bytes(rng.getrandbits(8) for _ in range(66000))
    return [case("stored isize %d" % n, dc.stored(noise[n % 97:n % 97 + n], True), text=noise[n % 97:n % 97 + n]) for n in SWEEP_SIZES]


@functools.lru_cache(None)
def cases_random(lo, hi):
    return [dict(zip(("member", "text"), dc.random_member(seed)), name="random_member seed %d" % seed) for seed in range(lo, hi)]


def _cut(ops, nbytes_hint):
    """the stream of one block, cut at a byte that lies inside a symbol and loses bits that are set"""
    full = dc.payload(ops)
    ends, at = set(), 0
    for _, n in ops:
        at += n
        ends.add(at)
    for keep in range(len(full) - nbytes_hint, 0, -1):
        if 8 * keep not in ends and any(full[keep:]):
            return full[:keep]
    raise AssertionError("no place to cut")


@functools.lru_cache(None)
def cases_refuse():
    """F. members that must be refused: [(name, member)]; every one alone in its call"""
    out = []
    text = lits(100)
    crc = zlib.crc32

    def bad(name, pay, claim=text, **kw):
        out.append((name, dc.member(pay, claim, **kw)))

    bad("R1 block type 3", dc.payload([(1, 1), (3, 2)], tail=text))
    bad("R2 NLEN mismatch", dc.payload(dc.stored(text, True, nlen=0x1234)))
    bad("R3 stored LEN past the payload", dc.payload([(1, 1), (0, 2), (0, -1), (100, 16), (100 ^ 0xFFFF, 16), (text[:10], -2)]))
    bad("R4 stored LEN past ISIZE", dc.payload(dc.stored(text, True)), text[:50])
    for f in (30, 31):
        bad("R5 HLIT field %d" % f, dc.payload([(1, 1), (2, 2), (f, 5), (0, 5), (15, 4)], tail=text))
        bad("R6 HDIST field %d" % f, dc.payload([(1, 1), (2, 2), (0, 5), (f, 5), (15, 4)], tail=text))
    tokens = [b"ABBA" * 25]
    ab = [0] * 257
    ab[65] = ab[66] = ab[256] = 1
    sent = {s for s, _ in dc._rle(sum(flat(tokens), []))}  # the code-length symbols these lengths are sent with
    assert 3 <= len(sent) < 8
    over_clen = [int(s in sent) for s in range(19)]
    bad("R7 over-subscribed code-length code", dc.payload(dc.dynamic(tokens, *flat(tokens), True, clen_lens=over_clen)), tokens[0])
    bad("R7 over-subscribed literal code", dc.payload(dc.dynamic(tokens, ab, [0], True)), tokens[0])
    m = [b"ABBA", (96, 2)]
    bad("R7 over-subscribed distance code", dc.payload(dc.dynamic(m, flat(m)[0], [1, 1, 1], True)), tokens[0])
    ok = dc._rle(flat(tokens)[0] + [0])
    bad("R8 code 16 first", dc.payload(dc.dynamic(tokens, *flat(tokens), True, rle=[(16, 0)] + ok)), tokens[0])
    bad("R9 repeat past HLIT + HDIST", dc.payload(dc.dynamic(tokens, *flat(tokens), True, rle=[(18, 127), (18, 127)])), tokens[0])
    no_eob = [0] * 257
    no_eob[65] = no_eob[66] = 1
    bad("R10 no end-of-block code", dc.payload(dc.dynamic(tokens, no_eob, [0], True)), tokens[0])
    bad("R10b HCLEN field 0: no length but 0 can be sent",
        dc.payload(dc.dynamic([], [0] * 257, [0], True, clen_lens=dc.flat_lens([0, 16, 17, 18], 19), hclen=4)), b"")
    for s in (286, 287):
        bad("R11 fixed-code symbol %d" % s, dc.payload(dc.fixed([text[:50], ("raw", s, 0, None, 0), text[50:]], True)))
    for s in (30, 31):
        bad("R12 fixed distance symbol %d" % s, dc.payload(dc.fixed([text[:50], ("raw", 257, 0, s, 0), text[53:]], True)))
    bad("R13 distance 1 at pos 0", dc.payload(dc.fixed([(3, 1), text[3:]], True)))
    bad("R13 distance pos + 1", dc.payload(dc.fixed([text[:50], (3, 51), text[53:]], True)))
    one = [text[:50], (3, 1), text[53:]]
    bad("R14 the unused code of a one-code distance tree",
        dc.payload(dc.dynamic([text[:50], ("raw", 257, 0, None, 0), ("bits", 1, 1), text[53:]], flat(one)[0], [1], True)))
    bad("R15 literal past ISIZE", dc.payload(dc.fixed([text], True)), text[:99])
    bad("R15 match ends past ISIZE", dc.payload(dc.fixed([text[:90], (10, 90)], True)), text[:99])
    bad("R15 stream short of ISIZE", dc.payload(dc.fixed([text[:99]], True)), text)
    bad("R16 fixed block cut inside a symbol", _cut(dc.fixed([text], True), 5))
    vcf = _vcf_text()[2000:4000]
    tokens = dc.tokenize(vcf, random.Random(5))
    bad("R16 dynamic block cut inside a symbol", _cut(dc.dynamic(tokens, *dc.random_lens(tokens, random.Random(6)), True), 9), vcf)
    bad("R17 right text, wrong CRC", dc.payload(dc.fixed([text], True)), crc=crc(text) ^ 0x00010000)
    return out


@functools.lru_cache(None)
def cases_lenient():
    """G. incomplete codes whose unused codes never occur: zlib refuses them, the device builds no completeness check"""
    out = []
    tokens = [lits(300), (258, 1), (40, 300), (3, 2), lits(5), (100, 77)]
    out.append(dyn_case("thirty 5-bit distance codes", tokens, (flat(tokens)[0], [5] * 30)))
    lit_lens = [0] * 257
    lit_lens[65] = lit_lens[66] = lit_lens[256] = 2
    out.append(dyn_case("literal code with Kraft sum 3/4", [b"ABBA" * 25], (lit_lens, [0])))
    tokens = [b"ABBA" * 25]
    sent = {s for s, _ in dc._rle(sum(flat(tokens), []))}  # the code-length symbols these lengths are sent with
    assert 2 <= len(sent) < 8
    clen = [3 * int(s in sent) for s in range(19)]
    out.append(dyn_case("incomplete code-length code", tokens, clen_lens=clen))
    return out


def fixture_members():
    """[(payload, crc, isize)] of tests/golden/libdeflate_members.bgzf"""
    with open(os.path.join(GOLDEN, "libdeflate_members.bgzf"), "rb") as f:
        data = f.read()
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append((data[at + 18:at + size - 8],) + struct.unpack_from("<II", data, at + size - 8))
        at += size
    assert at == len(data)
    return data, out


def zlib_inflate(pay):
    d = zlib.decompressobj(-15)
    text = d.decompress(pay)
    assert d.eof
    return text


# ------------------------------------------------------------------ the device
def check_group(bv, cases):
    """the members of a group in one call: one launch, and their odd sizes give every alignment of out_off"""
    comp = b"".join(c["member"] for c in cases)
    want = b"".join(c["text"] for c in cases)
    rc, text, n = bv.bgzf_inflate_device(comp, cap=len(want) + 64)
    if rc != 0:  # which one?  (valid members only: a refusal is a finding, not a fault)
        bad = [c["name"] for c in cases if bv.bgzf_inflate_device(c["member"], cap=len(c["text"]) + 64)[0] != 0]
        raise AssertionError("rc %d; refused alone: %s" % (rc, bad[:8]))
    if text != want:
        at = 0
        for c in cases:
            got = text[at:at + len(c["text"])]
            if got != c["text"]:
                k = next((i for i, (x, y) in enumerate(zip(got, c["text"])) if x != y), min(len(got), len(c["text"])))
                raise AssertionError("%s: text differs from byte %d of %d" % (c["name"], k, len(c["text"])))
            at += len(c["text"])
    assert n == len(want)


@pytest.mark.parametrize("W", (0,) + A_WINDOWS)
def test_match_placement(bv, W):
    check_group(bv, cases_a(W))


def test_codes(bv):
    check_group(bv, cases_b())


def test_blocks_and_sizes(bv):
    check_group(bv, cases_c())


def test_size_sweep(bv):
    check_group(bv, cases_sweep())


@pytest.mark.parametrize("lo", (0, 64, 128, 192))
def test_random_members(bv, lo):
    check_group(bv, cases_random(lo, lo + 64))


def test_libdeflate_fixture(bv):
    data, members = fixture_members()
    want = b"".join(zlib_inflate(pay) for pay, _, _ in members)
    rc, text, n = bv.bgzf_inflate_device(data, cap=len(want) + 64)
    assert rc == 0 and n == len(want)
    assert text == want


def libdeflate_texts():
    import test_gpu_inflate
    t = test_gpu_inflate._texts()
    return [t[k] for k in ("vcf", "random_small_alphabet", "long_lines", "bytes_all", "far_refs", "max", "period4_gt")] + \
        [_vcf_text()[:65536], lits(40000)]


def test_libdeflate_live(bv):
    import ctypes as C
    try:
        lib = C.CDLL("libdeflate.so.0")
    except OSError:
        pytest.skip("no libdeflate.so.0 on this machine")
    lib.libdeflate_alloc_compressor.restype = C.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [C.c_int]
    lib.libdeflate_deflate_compress.restype = C.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [C.c_void_p]
    cases = []
    for level in (0, 1, 6, 9, 12):
        comp = lib.libdeflate_alloc_compressor(level)
        assert comp
        for i, text in enumerate(libdeflate_texts()):
            buf = C.create_string_buffer(65510)
            n = lib.libdeflate_deflate_compress(comp, text, len(text), buf, len(buf))
            if n:  # (0: does not fit a member)
                assert zlib_inflate(buf.raw[:n]) == text
                cases.append(dict(name="libdeflate level %d text %d" % (level, i), member=dc.member(buf.raw[:n], text), text=text))
        lib.libdeflate_free_compressor(comp)
    assert len(cases) >= 40
    check_group(bv, cases)


def test_refused_members(bv):
    for name, member in cases_refuse():
        isize = struct.unpack("<I", member[-4:])[0]
        rc, _, _ = bv.bgzf_inflate_device(member, cap=isize + 64)
        assert rc == bv.E_FATAL, (name, rc)
    good = cases_c()[0]  # ... and the device is as it was
    rc, text, _ = bv.bgzf_inflate_device(good["member"], cap=len(good["text"]) + 64)
    assert rc == 0 and text == good["text"]


def test_lenient_members(bv):
    """(what the device does today is recorded in bvcf_inflate.hip.h's header comment)"""
    for c in cases_lenient():
        rc, text, _ = bv.bgzf_inflate_device(c["member"], cap=len(c["text"]) + 64)
        print("lenient: %s -> rc %d" % (c["name"], rc))
        assert rc == bv.E_FATAL or (rc == 0 and text == c["text"]), (c["name"], rc)


# ------------------------------------------------------------------ H. through the pipeline
NS = 150


@functools.lru_cache(None)
def cohort_vcf():
    import vcfgen
    return vcfgen.gen_vcf(355, 300, NS, weird=0.02)


def _members(data, sizes, blocks_of):
    """`data` cut into members of the given sizes of text (the last size repeats); blocks_of(tokens) -> deflate blocks"""
    out, at, k = [], 0, 0
    while at < len(data):
        n = sizes[min(k, len(sizes) - 1)]
        part = data[at:at + n]
        out.append(dc.member(dc.payload(*blocks_of(dc.tokenize(part, random.Random(k)), k)), part))
        at += n
        k += 1
    return out


def _blocks_random_codes(tokens, k):
    rng = random.Random(1000 + k)
    parts = [tokens[i:i + 200] for i in range(0, len(tokens), 200)] or [[]]
    return [dc.dynamic(p, *dc.random_lens(p, rng), i == len(parts) - 1) for i, p in enumerate(parts)]


def _blocks_in_turn(tokens, k):
    parts = [tokens[i:i + 150] for i in range(0, len(tokens), 150)] or [[]]
    blocks, text = [], bytearray()
    for i, p in enumerate(parts):
        at = len(text)
        dc.expand(p, text)
        blocks.append([dc.stored(text[at:], False), dc.fixed(p, False), dc.dynamic(p, *flat(p), False)][(i + k) % 3])
        blocks.append(dc.stored(b"", i == len(parts) - 1))
    return blocks


@functools.lru_cache(None)
def pipeline_files(data):
    """{name: [members]} -- `data` written three ways"""
    return {
        "random_codes": _members(data, [60000], _blocks_random_codes),
        "blocks_in_turn": _members(data, [24000], _blocks_in_turn),
        "member_sizes": _members(data, [65536, 1, 0, 20000, 0, 1, 1, 65536, 7777, 0, 30000], _blocks_random_codes),
    }


def _summary(b, body_of):
    lines, recs = [], []
    for i, L in enumerate(b.lines):
        st = int(L["status"])
        lines.append((st, body_of(b, i, L) if st in (0, 3) else None))
        recs.append([(int(r["alt_idx"]), int(r["ac"]), int(r["an"]), int(r["n_het"]), int(r["n_hom"]), int(r["n_miss"]))
                     for r in b.records(i)] if st == 0 else None)
    return lines, recs


@pytest.mark.parametrize("name", ["random_codes", "blocks_in_turn", "member_sizes"])
def test_submit_bgzf_of_crafted_files(bv, name):
    vcf = cohort_vcf()
    body = vcf[vcf.index(b"\n", vcf.index(b"#CHROM")) + 1:]
    ctx = bv.Ctx(9 + NS, allow="", max_batch_bytes=len(body) + 4096)
    want = _summary(ctx.process(body), lambda b, i, L: body[int(L["off"]):int(L["off"]) + min(int(L["fend"][7]), int(L["len"]))])
    ctx.close()
    comp = b"".join(pipeline_files(body)[name])
    ctx = bv.Ctx(9 + NS, allow="", max_batch_bytes=len(body) + (1 << 20))
    ctx.submit_bgzf(comp, len(comp), False)
    got = _summary(ctx.collect(), lambda b, i, L: b.line_head(i))
    ctx.close()
    assert len(got[0]) == body.count(b"\n")
    assert got[0] == want[0]
    assert got[1] == want[1]


def _cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")] + args, capture_output=True, timeout=120, env=e)


def _cli_equal(tmp_path, plain, comp):
    (tmp_path / "plain.vcf").write_bytes(plain)
    (tmp_path / "crafted.vcf.gz").write_bytes(comp)
    want = _cli(["--in", str(tmp_path / "plain.vcf")])
    assert want.returncode == 0 and want.stdout.count(b"\n") > 100
    for dev_inf in ("1", "0"):
        p = _cli(["--in", str(tmp_path / "crafted.vcf.gz")], {"BVCF_DEVICE_INFLATE": dev_inf})
        assert p.returncode == 0, (dev_inf, p.stderr[-300:])
        assert p.stdout == want.stdout, dev_inf
        assert p.stderr == want.stderr, dev_inf


@pytest.mark.parametrize("name", ["random_codes", "blocks_in_turn", "member_sizes"])
def test_cli_of_crafted_files(bv, tmp_path, name):
    import bgzf
    vcf = cohort_vcf()
    _cli_equal(tmp_path, vcf, b"".join(pipeline_files(vcf)[name]) + bgzf.bgzf_block(b""))


def test_cli_of_libdeflate_cohort(bv, tmp_path):
    import gzip
    import oracle_lib as orc
    with open(os.path.join(GOLDEN, "libdeflate_cohort.vcf.gz"), "rb") as f:
        comp = f.read()
    vcf = gzip.decompress(comp)
    rc_o, out_o, log_o, _ = orc.run(vcf)
    assert rc_o == 0
    (tmp_path / "cohort.vcf.gz").write_bytes(comp)
    for dev_inf in ("1", "0"):
        p = _cli(["--in", str(tmp_path / "cohort.vcf.gz")], {"BVCF_DEVICE_INFLATE": dev_inf})
        assert p.returncode == 0, (dev_inf, p.stderr[-300:])
        assert p.stdout == (bv.string_header() + "\n").encode() + out_o, dev_inf
        assert p.stderr.decode() == log_o, dev_inf
