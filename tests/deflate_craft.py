"""DEFLATE writer for tests (RFC 1951): streams built symbol by symbol, so that a test decides where every match, code
length and block boundary goes instead of taking what a compressor happens to emit.

A token is a literal byte (int), a run of literal bytes (bytes), a match (length, distance), a raw symbol pair
("raw", length_symbol, extra, distance_symbol | None, extra) for what no well-formed pair can say, or ("bits", value, n).  stored / fixed /
dynamic return a block as a list of (value, n_bits) writes -- (0, -1) pads to the byte, (bytes, -2) is whole bytes --,
payload() joins blocks into the bytes of a stream and member() frames a stream as a BGZF member."""
import bisect
import random
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0] * 4 + [e for e in range(1, 14) for _ in (0, 1)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
MAX_MEMBER = 65536  # bytes of a BGZF member (BSIZE is 16 bits) and the most text one may hold


class Bits:
    """LSB-first bit writer"""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << 8 * k) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def done(self):
        self.put(0, -self.n & 7)
        self.buf += self.acc.to_bytes(self.n >> 3, "little")
        self.acc = self.n = 0
        return bytes(self.buf)


def payload(*blocks, tail=b""):
    w = Bits()
    for block in blocks:
        for v, n in block:
            if n >= 0:
                w.put(v, n)
            else:
                w.done()
                if n == -2:
                    w.buf += v
    return w.done() + tail


def codes(lens):
    """the canonical code of every symbol (RFC 1951 3.2.2) as (bits reversed for the LSB-first stream, length) | None"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = code = 0
    nxt = [0] * 16
    for L in range(1, 16):
        code = (code + count[L - 1]) << 1
        nxt[L] = code
    out = []
    for l in lens:
        out.append((int(format(nxt[l] & ((1 << l) - 1), "0%db" % l)[::-1], 2), l) if l else None)
        nxt[l] += 1
    return out


def match_syms(length, dist):
    ls, ds = bisect.bisect_right(LEN_BASE, length) - 1, bisect.bisect_right(DIST_BASE, dist) - 1
    return 257 + ls, length - LEN_BASE[ls], ds, dist - DIST_BASE[ds]


def raw_of(t):
    return t[1:] if t[0] == "raw" else match_syms(*t)


def symbols(tokens):
    """(literal/length symbols, distance symbols) the tokens use, the end-of-block code included"""
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        elif isinstance(t, bytes):
            lit.update(t)
        elif t[0] != "bits":
            ls, _, ds, _ = raw_of(t)
            lit.add(ls)
            dist.add(ds)
    return lit, dist - {None}


def expand(tokens, out=None):
    """the plain definition of what the tokens mean (continuing the text `out`)"""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, bytes):
            out += t
        else:
            ls, lx, ds, dx = raw_of(t)
            length, dist = LEN_BASE[ls - 257] + lx, DIST_BASE[ds] + dx
            assert 3 <= length <= 258 and 1 <= dist <= min(len(out), 32768), t
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
    return out


_FIXED8 = bytes(int(format(0x30 + b, "08b")[::-1], 2) if b < 144 else 0 for b in range(256))


def _sym_writes(tokens, lit, dist, fixed_code=False):
    ops = []
    for t in tokens:
        if isinstance(t, int):
            ops.append(lit[t])
        elif isinstance(t, bytes):
            if fixed_code and t and max(t) < 144:  # eight bits each: the whole run in one write
                ops.append((int.from_bytes(t.translate(_FIXED8), "little"), 8 * len(t)))
            else:
                ops.extend(lit[b] for b in t)
        elif t[0] == "bits":
            ops.append(t[1:])
        else:
            ls, lx, ds, dx = raw_of(t)
            ops.append(lit[ls])
            ops.append((lx, LEN_EXTRA[ls - 257] if ls < 286 else 0))
            if ds is not None:
                ops.append(dist[ds])
                ops.append((dx, DIST_EXTRA[ds] if ds < 30 else 0))
    if lit[256]:
        ops.append(lit[256])
    return ops


def stored(data, last, nlen=None):
    n = len(data)
    return [(int(last), 1), (0, 2), (0, -1), (n, 16), ((n ^ 0xFFFF) if nlen is None else nlen, 16), (bytes(data), -2)]


def fixed(tokens, last):
    return [(int(last), 1), (1, 2)] + _sym_writes(tokens, codes(FIXED_LIT), codes(FIXED_DIST), True)


def flat_lens(syms, size):
    """a complete code, as flat as it can be, over `syms` of an alphabet of `size` (one symbol: a single 1-bit code)"""
    syms, lens = sorted(syms), [0] * size
    L = max(1, (len(syms) - 1).bit_length())
    for i, s in enumerate(syms):
        lens[s] = L - 1 if len(syms) > 1 and i < (1 << L) - len(syms) else L
    return lens


def _rle(seq):
    items, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        run = j - i
        if seq[i] == 0 and run >= 3:
            n = min(run, 138)
            items.append((17, n - 3) if n <= 10 else (18, n - 11))
        elif i and seq[i] == seq[i - 1] and run >= 3:
            n = min(run, 6)
            items.append((16, n - 3))
        else:
            n = 1
            items.append((seq[i], 0))
        i += n
    return items


def dynamic(tokens, lit_lens, dist_lens, last, clen_lens=None, rle=True, hclen=19):
    """rle: True = repeat codes where they fit, False = none, or the (code-length symbol, extra) items themselves"""
    seq = list(lit_lens) + list(dist_lens)
    items = _rle(seq) if rle is True else ([(l, 0) for l in seq] if rle is False else list(rle))
    if clen_lens is None:
        used = {s for s, _ in items}
        clen_lens = flat_lens(used if len(used) > 1 else used | {17, 18}, 19)
    assert not any(clen_lens[s] for s in CLEN_ORDER[hclen:])
    cc = codes(clen_lens)
    ops = [(int(last), 1), (2, 2), (len(lit_lens) - 257, 5), (len(dist_lens) - 1, 5), (hclen - 4, 4)]
    ops += [(clen_lens[s], 3) for s in CLEN_ORDER[:hclen]]
    for s, x in items:
        ops += [cc[s], (x, (2, 3, 7)[s - 16] if s >= 16 else 0)]
    return ops + _sym_writes(tokens, codes(lit_lens), codes(dist_lens))


def member(payload_bytes, text, crc=None, isize=None):
    """a BGZF member around a deflate stream; crc / isize: what the trailer claims, if not the text's"""
    bsize = len(payload_bytes) + 25  # header 18 + payload + crc 4 + isize 4 - 1
    assert bsize < 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize) + payload_bytes +
            struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize))


def random_code(syms, rng, max_len=15):
    """{symbol: length} of a random COMPLETE prefix code: the leaves of a random binary tree no deeper than max_len"""
    syms = list(syms)
    assert 2 <= len(syms) <= 1 << max_len
    depths = [1, 1]
    while len(depths) < len(syms):
        can = [i for i, d in enumerate(depths) if d < max_len]
        i = rng.choice(can) if rng.random() < 0.6 else max(can, key=depths.__getitem__)  # (some trees grow one long arm)
        d = depths.pop(i) + 1
        depths += [d, d]
    rng.shuffle(syms)
    return dict(zip(syms, depths))


def random_lens(tokens, rng, max_len=15):
    """(lit_lens, dist_lens) of random complete codes over what the tokens use; a lone distance symbol keeps a 1-bit
    code or gets a partner, no distance at all is HDIST = 1 with length 0"""
    lit, dist = symbols(tokens)
    if len(lit) < 2:
        lit = lit | {rng.randrange(256)}
    if len(dist) == 1 and rng.random() < 0.5:
        dist = dist | {(min(dist) + 1 + rng.randrange(29)) % 30}
    lc = random_code(lit, rng, max_len)
    dc = random_code(dist, rng, max_len) if len(dist) > 1 else {d: 1 for d in dist}
    return [lc.get(s, 0) for s in range(max(lit) + 1 if max(lit) > 256 else 257)], [dc.get(s, 0) for s in range(max(dist, default=0) + 1)]


def tokenize(data, rng, max_dist=32768):
    """greedy matcher over a hash of three bytes; now and then it passes a match by or cuts it short"""
    data, out, seen, i, n = bytes(data), [], {}, 0, len(data)
    while i < n:
        best = bd = 0
        for j in seen.get(data[i:i + 3], ())[-6:]:
            if i - j <= max_dist and i + 3 <= n:
                lo, hi = 3, min(258, n - i)
                while lo < hi:  # the longest common run, by bisection over slices
                    mid = (lo + hi + 1) // 2
                    lo, hi = (mid, hi) if data[j:j + mid] == data[i:i + mid] else (lo, mid - 1)
                if lo > best:
                    best, bd = lo, i - j
        r = rng.random()
        if best >= 3 and r >= 0.05:
            if r < 0.1:
                best = rng.randint(3, best)
            out.append((best, bd))
        else:
            out.append(data[i])
            best = 1
        for k in range(i, i + best):
            seen.setdefault(data[k:k + 3], []).append(k)
        i += best
    return out


EDGE_DISTS = [w + d for w in (4096, 16384, 32768) for d in (-259, -257, -66, -4, -3, -2, -1, 0, 1, 2, 3) if w + d <= 32768]
EDGE_LENS = [3, 4, 63, 64, 65, 66, 257, 258]


def random_member(seed):
    """-> (BGZF member, its text): random tokens, cut into 1..12 blocks of random kind"""
    rng = random.Random(seed)
    alphabet = b"01|/.\t\n:,ACGT" * 6 + bytes(rng.randrange(256) for _ in range(rng.choice([0, 4, 40])))
    target = rng.choice([rng.randint(1, 300), 5000, 20000, 40000, MAX_MEMBER - rng.randint(0, 3), MAX_MEMBER])
    tokens, pos = [], 0
    while pos < target and len(tokens) < 2500:
        if pos == 0 or rng.random() < 0.35:
            t = bytes(rng.choice(alphabet) for _ in range(min(rng.choice([1, 1, 2, 5, 19]), target - pos)))
            tokens.append(t if len(t) > 1 else t[0])
            pos += len(t)
            continue
        dist = rng.choice([1, 2, 3, 4, 8, rng.choice(EDGE_DISTS), rng.choice(EDGE_DISTS), rng.randint(1, 32768)])
        length = min(rng.choice(EDGE_LENS + [rng.randint(3, 258), 258, 258]), target - pos)
        if length < 3:
            continue
        tokens.append((length, min(dist, pos)))
        pos += length
    cuts = sorted(rng.sample(range(1, len(tokens)), min(rng.randint(0, 11), len(tokens) - 1)))
    blocks, text = [], bytearray()
    for k, (a, b) in enumerate(zip([0] + cuts, cuts + [len(tokens)])):
        part, last, at = tokens[a:b], b == len(tokens), len(text)
        expand(part, text)
        kind = rng.choice(["stored", "fixed", "dynamic", "dynamic"])
        if kind == "stored" and len(text) - at <= 3000:
            blocks.append(stored(text[at:], last))
        elif kind == "fixed":
            blocks.append(fixed(part, last))
        else:
            blocks.append(dynamic(part, *random_lens(part, rng), last))
    return member(payload(*blocks), bytes(text)), bytes(text)
