"""k_stream's pending-store log (the pipelined path: lines of <= 10 chunks, one-byte line end): entries, head bitmaps,
ALT #1's class lists and dense maps wait in LDS as 16-byte pieces -- 150 fit -- and leave together when the largest line
of the geometry would no longer fit behind them, at every exit from the pipeline, ahead of the stores the pipeline still
makes directly, and at the wall-clock epochs.  Results are where they always were, so every case is
the streaming path through the library against the oracle, byte for byte.

Pieces per line: entry 2, head bitmap 2 (not on the first line of a pipeline run), a class list of n entries
(n + 4) // 4 (n <= 15), a dense map of 2 504 samples 40."""
import random

import pytest

import vcfgen
from test_gpu_parity import both

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def streaming_path(monkeypatch):
    monkeypatch.setenv("BVCF_PATH", "2")
    monkeypatch.setenv("BVCF_GEN_STREAM", "0")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def row(rng, ns, pos, k, alt="G", gts_alt=("0|1", "1|0", "1|1", ".|."), fmt="GT", id_len=None):
    """a regular line whose class list has k entries: k of the (ns + 3) // 4 four-sample lanes hold a non-reference field"""
    gts = ["0|0"] * ns
    for b in rng.sample(range((ns + 3) // 4), min(k, (ns + 3) // 4)):
        for q in rng.sample(range(4), rng.randint(1, 4)):
            if 4 * b + q < ns:
                gts[4 * b + q] = rng.choice(gts_alt)
        if all(g == "0|0" for g in gts[4 * b:4 * b + 4]):
            gts[min(4 * b, ns - 1)] = gts_alt[0]
    # (the ID's length moves the sample region over the four byte alignments)
    rid = "r" + "x" * (rng.randint(0, 3) if id_len is None else id_len)
    return "\t".join(["7", str(pos), rid, "A", alt, "50", "PASS", "AC=1", fmt] + gts) + "\n"


def vcf_of(ns, ks, seed=1, **kw):
    rng = random.Random(seed)
    return (vcfgen.header(ns) + "".join(row(rng, ns, 1000 + 3 * i, k, **kw) for i, k in enumerate(ks))).encode()


def body_of(vcf):
    hdr_at = vcf.index(b"#CHROM")
    hdr_end = vcf.index(b"\n", hdr_at)
    return vcf[hdr_at:hdr_end].count(b"\t") + 1, vcf[hdr_end + 1:]


def test_log_overflow(bv):
    """40 dense maps back to back (44 pieces each: the log holds three), then sparse lines"""
    both(bv, vcf_of(2504, [70] * 40 + [0, 1, 2, 5, 3, 0] * 10))


@pytest.mark.parametrize("tail", [(1, 2, 13), (1, 5, 13), (1, 2, 9), (0, 0, 0, 1)])
def test_exactly_at_capacity(bv, tail):
    """2 504 samples: the largest line is 44 pieces, so the log leaves once more than 106 wait.  Two or three dense lines
    (88 / 132 pieces, two less when the first opens the pipeline run) and lists of 5 + 5 + 8, 5 + 6 + 8, 5 + 5 + 7 and
    5 + 5 + 5 + 5 pieces behind them; the pattern repeats, so that it meets the log at every fill -- 106 and 107 among them"""
    both(bv, vcf_of(2504, ([70, 80, 64] + list(tail)) * 12, seed=len(tail) + tail[1]))
    both(bv, vcf_of(2504, ([70, 80] + list(tail)) * 12, seed=len(tail) + tail[1] + 1))


def test_log_filled_to_the_last_piece(bv):
    """255 samples: a line is 8 pieces at most (a map of 64 bytes), so the log leaves once more than 142 wait, and lines of
    5..8 pieces (lists of 0..15 entries, maps) fill it to every count up to 150, the last piece included"""
    rng = random.Random(77)
    both(bv, vcf_of(255, [rng.choice([0, 2, 4, 5, 8, 11, 12, 15, 16, 30]) for _ in range(600)], seed=78))


def test_lists_of_every_size_and_zero_fill(bv):
    """0, 1, 3, 4, 7, 8, 11, 12 and 15 entries: every piece count of a list; the dwords between a list's last entry
    and the end of its last piece are zero"""
    sizes = [0, 1, 3, 4, 7, 8, 11, 12, 15]
    vcf = vcf_of(2504, sizes * 8 + sizes[::-1] * 4, seed=3)
    both(bv, vcf)
    n_header, body = body_of(vcf)
    ctx = bv.Ctx(n_header)
    b = ctx.process(body)
    ctx.close()
    seen = set()
    for i in range(len(b.lines)):
        if int(b.lines[i]["n_rec"]) == 0:
            continue
        rec = b.records(i)[0]
        assert int(rec["flags"]) & 2, "a line of <= 15 entries comes back as a class list"
        off = int(rec["cmap_off"])
        words = b.cmap[off:off + 64].view("<u4")
        n = int(words[0])
        seen.add(n)
        assert not words[n + 1:4 * ((n + 4) // 4)].any(), (i, n, words.tolist())
    assert seen >= set(sizes) - {0}


def test_list_to_map_boundary(bv):
    """15 entries are a list, 16 and 63 a map built at the line's end, 64 one that went dense on the way"""
    both(bv, vcf_of(2504, [15, 16, 63, 64, 16, 15, 63, 0, 16, 64, 17] * 6, seed=4))
    both(bv, vcf_of(300, [15, 16, 63, 64, 16, 15, 63, 0, 16, 64, 17] * 6, seed=5))


@pytest.mark.parametrize("k", [1, 2, 5])
def test_malformed_field_leaves_the_pipeline(bv, k):
    """a sample field that is no genotype (same length: the line still looks regular until it is scanned) k lines after
    a run of dense lines that has just overflowed the log: the pipeline is left with entries pending"""
    rng = random.Random(10 + k)
    ns = 2504
    rows, pos = [vcfgen.header(ns)], 100
    for rep in range(14):
        for kk in [70, 66, 90] + [rng.randint(0, 15) for _ in range(k - 1)]:
            pos += 5
            rows.append(row(rng, ns, pos, kk))
        pos += 5
        bad = row(rng, ns, pos, 3).rstrip("\n").split("\t")
        bad[9 + rng.randrange(ns)] = rng.choice(["0|x", "0:1", "|01", "1|:"])
        rows.append("\t".join(bad) + "\n")
    both(bv, "".join(rows).encode(), {"allow": ""})


def test_other_shape_unterminated_and_cut_lines(bv, monkeypatch):
    ns = 2504
    rng = random.Random(21)
    ks = [rng.choice([0, 2, 7, 15, 16, 70]) for _ in range(90)]
    rows = [row(rng, ns, 1000 + 3 * i, k) for i, k in enumerate(ks)]
    # GT:DP lines in between: longer than 4 ns bytes, the predicted line end holds no terminator
    for i in range(5, len(rows), 9):
        f = rows[i].rstrip("\n").split("\t")
        rows[i] = "\t".join(f[:8] + ["GT:DP"] + [g + ":%d" % rng.randint(0, 30) for g in f[9:]]) + "\n"
    vcf = (vcfgen.header(ns) + "".join(rows)).encode()
    both(bv, vcf, {"allow": ""})
    both(bv, vcf[:-1], {"allow": ""})                       # an unterminated last line
    both(bv, vcf[:-1 - 4 * 1000], {"allow": ""})            # ... that ends inside its sample region
    # tiny tiles: the cut line is the first (and only) line of some wave's run
    monkeypatch.setenv("BVCF_TILE_KB", "4")
    both(bv, vcf[:-1 - 4 * 1000], {"allow": ""})
    both(bv, vcf[:-1 - 10000], {"allow": ""})               # ... and inside its head


@pytest.mark.parametrize("ns", [255, 256, 260, 1030, 2560, 4097])
def test_geometry(bv, ns):
    """1..10 chunks per line (256 and 2 560 samples: the unaligned loads), and 17 chunks: no room for a log beside the
    stage, every store direct"""
    rng = random.Random(ns)
    ks = [rng.choice([0, 1, 4, 15, 16, 40, 64, 200]) for _ in range(150 if ns < 1100 else 60)]
    both(bv, vcf_of(ns, ks, seed=ns, alt="C,G", gts_alt=("0|1", "1|1", ".|.", "1|.", "2|1")))


def test_lines_cross_tiles_while_pending(bv, monkeypatch):
    monkeypatch.setenv("BVCF_TILE_KB", "4")
    rng = random.Random(31)
    for ns in (300, 1030, 2504):
        ks = [rng.choice([0, 1, 3, 8, 15, 16, 70]) for _ in range(200 if ns < 2000 else 120)]
        vcf = vcf_of(ns, ks, seed=ns + 1)
        both(bv, vcf)
        both(bv, vcf, max_batch_bytes=1 << 20)


def test_multiallelic_between_pending_lines(bv):
    """further alleles' lists (few carriers), a raw list behind the slot (16..63 non-reference lanes, or a dense line with
    a few carriers of ALT #2) and lines left to k_gt, between plain lines whose stores are pending"""
    rng = random.Random(41)
    ns = 2504
    rows, pos = [vcfgen.header(ns)], 500
    for i in range(160):
        pos += 4
        kind = i % 8
        if kind in (1, 5):
            rows.append(row(rng, ns, pos, rng.choice([2, 9, 14]), alt="G,T,C", gts_alt=("0|1", "2|1", "0|2", "3|3", ".|2")))
        elif kind == 3:
            rows.append(row(rng, ns, pos, rng.choice([20, 40, 63]), alt="G,T", gts_alt=("0|1", "1|1", "0|2", "2|2")))
        elif kind == 6:
            f = row(rng, ns, pos, 120, alt="G,T").rstrip("\n").split("\t")
            for s in rng.sample(range(ns), 5):
                f[9 + s] = rng.choice(["0|2", "2|1", "2|2"])
            rows.append("\t".join(f) + "\n")
        else:
            rows.append(row(rng, ns, pos, rng.choice([0, 1, 6, 15, 70])))
    both(bv, "".join(rows).encode())


def _same_batch(a, b):
    """(not the class-map offsets themselves: another ctx splits the block over another number of waves, whose slots they
    are, and the maps of further alleles are handed out in the order their lines are reached)"""
    assert len(a.lines) == len(b.lines) and len(a.alleles) == len(b.alleles)
    for f in ("off", "len", "n_rec", "status", "n_fields"):
        assert (a.lines[f] == b.lines[f]).all(), f
    ns = a.n_samples
    for i in range(len(a.lines)):
        # (through records(): alleles[] slots without a record hold nothing)
        ra, rb = a.records(i), b.records(i)
        for f in ("pos", "alt_idx", "ac", "an", "n_het", "n_hom", "n_miss", "ref", "kind", "trtv", "flags"):
            assert (ra[f] == rb[f]).all(), (i, f)
        for rec, rec_b in zip(a.records(i), b.records(i)):
            off, off_b = int(rec["cmap_off"]), int(rec_b["cmap_off"])
            assert (off == 0xFFFFFFFF) == (off_b == 0xFFFFFFFF)
            if off == 0xFFFFFFFF:
                continue
            if int(rec["flags"]) & 2:
                n = 4 * (1 + int(a.cmap[off:off + 4].view("<u4")[0]))
            else:
                n = (ns + 3) // 4
            assert (a.cmap[off:off + n] == b.cmap[off_b:off_b + n]).all(), (i, off, off_b)


def test_stability_two_batches_in_flight(bv):
    """two batches in flight on three slots, each compared with the same bytes processed alone and with the oracle; the
    same input twice: identical entries and identical class-map bytes at every record's offset"""
    rng = random.Random(51)
    ns = 2504
    parts = []
    for seed in (1, 2):
        ks = [rng.choice([0, 1, 3, 8, 15, 16, 63, 70]) for _ in range(150)]
        parts.append(vcf_of(ns, ks, seed=50 + seed, alt="G,T", gts_alt=("0|1", "1|1", ".|.", "0|2")))
    for v in parts:
        both(bv, v)
    n_header, body1 = body_of(parts[0])
    _, body2 = body_of(parts[1])
    one = bv.Ctx(n_header, n_slots=1)
    alone = [one.process(body1), one.process(body2)]
    one.close()
    ctx = bv.Ctx(n_header, n_slots=3)
    for rnd in range(2):
        ctx.submit(body1, seq=2 * rnd)
        keep = body1
        ctx.submit(body2, seq=2 * rnd + 1)
        got1 = ctx.collect()
        got2 = ctx.collect()
        del keep
        _same_batch(alone[0], got1)
        _same_batch(alone[1], got2)
    again = ctx.process(body1)
    _same_batch(got1, again)
    ctx.close()
