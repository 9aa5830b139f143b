"""The other half of deflate_craft.py, for the tests of the device compressor (bvcf_deflate.hip.h): a DEFLATE reader that
keeps every token and every header field of every block, and plain sequential references of what k_deflate is meant to
compute -- its tokens (steps 1 and 2 of its header comment), optimal and length-limited code costs, the run-length rule
of the block header, and the sizes of the three block forms.  Pure Python, tables from deflate_craft."""
import heapq

import deflate_craft as dc

PIECE = 65280
MAX_MATCH, MAX_DIST, CHUNK, HASH_BITS = 258, 32768, 256, 14
STORED, FIXED, DYNAMIC = 0, 1, 2
LL_EXTRA = [0] * 257 + dc.LEN_EXTRA  # extra bits of every literal/length symbol
RLE_EXTRA = {16: 2, 17: 3, 18: 7}


# ---- the reader

class _In:
    def __init__(self, data):
        self.d, self.pos = bytes(data) + b"\0\0\0\0", 0
        self.end = 8 * len(data)

    def peek(self):  # >= 25 bits from the position on
        return int.from_bytes(self.d[self.pos >> 3:(self.pos >> 3) + 4], "little") >> (self.pos & 7)

    def take(self, n):
        v = self.peek() & ((1 << n) - 1)
        self.pos += n
        assert self.pos <= self.end, "the stream ends inside a block"
        return v


def _table(lens):
    """(table over the next `width` bits -> (symbol, length), width); the code may be incomplete but not over-subscribed"""
    width = max(lens) if any(lens) else 1
    assert sum(1 << (width - l) for l in lens if l) <= 1 << width, "over-subscribed code"
    tab = [None] * (1 << width)
    for s, c in enumerate(dc.codes(lens)):
        if c:
            for k in range(c[0], 1 << width, 1 << c[1]):
                tab[k] = (s, c[1])
    return tab, width


def _symbol(r, tab, width):
    e = tab[r.peek() & ((1 << width) - 1)]
    assert e is not None, "a code that no symbol has"
    r.pos += e[1]
    assert r.pos <= r.end, "the stream ends inside a block"
    return e[0]


_FIXED_TABS = None


def read_blocks(payload):
    """raw DEFLATE -> (records, bits consumed).  A record: bfinal, btype, tokens (a literal byte or (length, distance)),
    bits (of this block, a stored block's padding included); dynamic blocks also hlit, hdist, hclen, clen_lens (19, by
    symbol), rle (the entries as sent: (symbol, extra value)), lit_lens (hlit of them), dist_lens (hdist)"""
    global _FIXED_TABS
    r, out = _In(payload), []
    while True:
        start = r.pos
        rec = {"bfinal": r.take(1), "btype": r.take(2)}
        assert rec["btype"] != 3, "block type 3"
        if rec["btype"] == STORED:
            r.pos = (r.pos + 7) & ~7
            at = r.pos >> 3
            n, nn = int.from_bytes(r.d[at:at + 2], "little"), int.from_bytes(r.d[at + 2:at + 4], "little")
            assert n ^ nn == 0xFFFF and 8 * (at + 4 + n) <= r.end, "stored block"
            rec["tokens"] = list(r.d[at + 4:at + 4 + n])
            r.pos = 8 * (at + 4 + n)
        else:
            if rec["btype"] == FIXED:
                if _FIXED_TABS is None:
                    _FIXED_TABS = _table(dc.FIXED_LIT), _table(dc.FIXED_DIST)
                lt, dt = _FIXED_TABS
            else:
                hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
                assert hlit <= 286 and hdist <= 30
                clen = [0] * 19
                for s in dc.CLEN_ORDER[:hclen]:
                    clen[s] = r.take(3)
                ct, seq, rle = _table(clen), [], []
                while len(seq) < hlit + hdist:
                    s = _symbol(r, *ct)
                    x = r.take(RLE_EXTRA[s]) if s >= 16 else 0
                    rle.append((s, x))
                    if s == 16:
                        assert seq, "repeat with nothing before it"
                        seq += [seq[-1]] * (3 + x)
                    else:
                        seq += [s] if s < 16 else [0] * ((3 if s == 17 else 11) + x)
                assert len(seq) == hlit + hdist, "a run past the last code length"
                rec.update(hlit=hlit, hdist=hdist, hclen=hclen, clen_lens=clen, rle=rle, lit_lens=seq[:hlit], dist_lens=seq[hlit:])
                assert seq[256], "no end-of-block code"
                lt, dt = _table(seq[:hlit]), _table(seq[hlit:])
            toks = rec["tokens"] = []
            while True:
                s = _symbol(r, *lt)
                if s < 256:
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    assert s < 286, "length symbol 286 / 287"
                    length = dc.LEN_BASE[s - 257] + r.take(dc.LEN_EXTRA[s - 257])
                    d = _symbol(r, *dt)
                    assert d < 30, "distance symbol 30 / 31"
                    toks.append((length, dc.DIST_BASE[d] + r.take(dc.DIST_EXTRA[d])))
        rec["bits"] = r.pos - start
        out.append(rec)
        if rec["bfinal"]:
            return out, r.pos


def expand(records):
    text = bytearray()
    for rec in records:
        dc.expand(rec["tokens"], text)
    return bytes(text)


def histograms(tokens):
    """(hll[286], hd[30]) of a token list, its one end-of-block code included"""
    hll, hd = [0] * 286, [0] * 30
    hll[256] = 1
    for t in tokens:
        if isinstance(t, int):
            hll[t] += 1
        else:
            ls, _, ds, _ = dc.match_syms(*t)
            hll[ls] += 1
            hd[ds] += 1
    return hll, hd


# ---- the reference tokenizer: steps 1 and 2 of k_deflate's header comment, one position after the other

def hash4(t, p):
    return ((int.from_bytes(t[p:p + 4], "little") * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def candidate(t, p):
    """the table entry position p of a piece looks at: the latest position of the chunks before p's with p's hash, or None"""
    h = hash4(t, p)
    return next((q for q in range(min(p - p % CHUNK, len(t) - 3) - 1, -1, -1) if hash4(t, q) == h), None)


def tokenize(t):
    """the greedy parse from position 0 over k_deflate's matches: the candidate of a position is the latest position of
    EARLIER 256-position chunks with its hash, it counts if it is within 32 768 and equal on 4 bytes, and the match runs
    to the first mismatch, 258 bytes or the end of the piece"""
    t = bytes(t)
    n = len(t)
    assert n <= PIECE
    tab, out, x = {}, [], 0
    for c0 in range(0, n, CHUNK):
        c1 = min(n, c0 + CHUNK)
        while x < c1:
            q = tab.get(hash4(t, x)) if x + 4 <= n else None
            if q is not None and x - q <= MAX_DIST and t[q:q + 4] == t[x:x + 4]:
                lim = min(MAX_MATCH, n - x)
                a, b = t[q:q + lim], t[x:x + lim]
                length = lim if a == b else next(i for i in range(4, lim) if a[i] != b[i])
                out.append((length, x - q))
                x += length
            else:
                out.append(t[x])
                x += 1
        for p in range(c0, min(c1, n - 3)):
            tab[hash4(t, p)] = p
    return out


# ---- reference codes

def huffman_depths(freqs):
    """{symbol: depth} of a Huffman tree over the symbols with freqs[s] > 0, unlimited; among the optimal trees the one
    that is least deep (ties go to the shallower subtree).  One symbol: depth 1"""
    heap = [(f, 0, s, (s,)) for s, f in enumerate(freqs) if f]
    depth = {e[2]: 0 for e in heap}
    if len(heap) == 1:
        return {heap[0][2]: 1}
    heapq.heapify(heap)
    tick = len(freqs)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[3] + b[3]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tick, a[3] + b[3]))
        tick += 1
    return depth


def cost(freqs, lens):
    return sum(f * lens[s] for s, f in enumerate(freqs) if f)


def huffman_cost(freqs):
    d = huffman_depths(freqs)
    return sum(freqs[s] * d[s] for s in d), max(d.values(), default=0)


def package_merge(freqs, limit):
    """{symbol: length} of an optimal prefix code with no length over `limit` (Larmore & Hirschberg's package-merge)"""
    syms = sorted((s for s, f in enumerate(freqs) if f), key=lambda s: (freqs[s], s))
    n = len(syms)
    if n == 1:
        return {syms[0]: 1}
    assert n <= 1 << limit
    leaves = [(freqs[s], [i == j for j in range(n)]) for i, s in enumerate(syms)]
    prev = leaves
    for _ in range(limit - 1):
        packs = [(prev[k][0] + prev[k + 1][0], [x + y for x, y in zip(prev[k][1], prev[k + 1][1])]) for k in range(0, len(prev) - 1, 2)]
        prev = sorted(leaves + packs, key=lambda e: e[0])
    lens = [0] * n
    for _, cnt in prev[:2 * n - 2]:
        lens = [x + y for x, y in zip(lens, cnt)]
    return {s: lens[i] for i, s in enumerate(syms)}


def limited_cost(freqs, limit):
    pm = package_merge(freqs, limit)
    return sum(freqs[s] * l for s, l in pm.items())


def kraft(lens, limit=15):
    """the Kraft sum in units of 2^-limit"""
    return sum(1 << (limit - l) for l in lens if l)


def rle_rule(seq):
    """the run-length entries (symbol, extra value) of a sequence of code lengths, as k_deflate's comment states the
    rule: a run of zeros gives 18 while 11 or more are left (at most 138 each), then 17 for 3 to 10, then single zeros;
    a run of another value gives the value once, then 16 while 3 or more are left (at most 6 each), then single values"""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
        out += [(v, 0)] * run
    return out


def trim(lit_lens, dist_lens):
    """(hlit, hdist): the fewest lengths that may be sent"""
    hlit, hdist = 286, 30
    while hlit > 257 and not lit_lens[hlit - 1]:
        hlit -= 1
    while hdist > 1 and not dist_lens[hdist - 1]:
        hdist -= 1
    return hlit, hdist


def min_hclen(clen_lens):
    h = 19
    while h > 4 and not clen_lens[dc.CLEN_ORDER[h - 1]]:
        h -= 1
    return h


def header_bits(hclen, clen_lens, rle):
    return 3 + 14 + 3 * hclen + sum(clen_lens[s] + RLE_EXTRA.get(s, 0) for s, _ in rle)


def body_bits(hll, hd, lit_lens, dist_lens):
    return (sum(f * (lit_lens[s] + LL_EXTRA[s]) for s, f in enumerate(hll) if f) +
            sum(f * (dist_lens[s] + dc.DIST_EXTRA[s]) for s, f in enumerate(hd) if f))


def fixed_bytes(hll, hd):
    return (3 + body_bits(hll, hd, dc.FIXED_LIT, dc.FIXED_DIST) + 7) >> 3


def choose(n, dyn_b, fix_b):
    """the block form of a piece of n bytes: stored wins its ties, then fixed wins its tie with dynamic"""
    sto_b = n + 5
    if sto_b <= dyn_b and sto_b <= fix_b:
        return STORED, sto_b
    return (FIXED, fix_b) if fix_b <= dyn_b else (DYNAMIC, dyn_b)


def reference_sizes(hll, hd, n):
    """(kind, dyn_b, fix_b, header bits, clen histogram) of the block of these histograms under Huffman depths from
    huffman_depths.  The sizes are those of ANY optimal code builder where the literal/length and distance lengths are
    forced (dyadic or flat frequencies: then the header is one sequence) and the code-length code needs no limiting (its
    cost is the same for every Huffman tree)"""
    def lens_of(freqs, size):
        d = huffman_depths(freqs)
        if len(d) < 2:  # the two-code minimum
            d = {next(iter(d), 0): 1, (0 if next(iter(d), 0) else 1): 1}
        return [d.get(s, 0) for s in range(size)]
    lit, dist = lens_of(hll, 286), lens_of(hd, 30)
    assert max(lit) <= 15 and max(dist) <= 15
    hlit, hdist = trim(lit, dist)
    rle = rle_rule(lit[:hlit] + dist[:hdist])
    fcl = [0] * 19
    for s, _ in rle:
        fcl[s] += 1
    ccost, cdepth = huffman_cost(fcl)
    assert cdepth <= 7
    hclen = min_hclen(fcl)
    hdr = 3 + 14 + 3 * hclen + ccost + sum(RLE_EXTRA.get(s, 0) for s, _ in rle)
    dyn_b = (hdr + body_bits(hll, hd, lit, dist) + 7) >> 3
    fix_b = fixed_bytes(hll, hd)
    return choose(n, dyn_b, fix_b)[0], dyn_b, fix_b, hdr, fcl


def check_lengths(freqs, lens, limit, label=""):
    """what every tree k_deflate builds must satisfy, whatever its shape: no length over the limit, exactly the used
    symbols coded (zlib's two-code minimum apart), a Kraft sum of exactly 1.  -> the code's cost"""
    used = [s for s, f in enumerate(freqs) if f]
    assert max(lens) <= limit, label
    if len(used) >= 2:
        assert [s for s, l in enumerate(lens) if l] == used, label
    elif len(used) == 1:  # the symbol and a partner: symbol 0, or 1 if the symbol is 0
        assert [s for s, l in enumerate(lens) if l] == sorted([used[0], 0 if used[0] else 1]), label
    else:
        assert [s for s, l in enumerate(lens) if l] == [0, 1], label
    assert kraft(lens, limit) == 1 << limit, label
    return cost(freqs, lens)
