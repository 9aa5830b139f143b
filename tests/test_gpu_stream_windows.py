"""k_stream's pending-store log leaves at chip-wide epochs of the wall clock (KernelArgs.pend_epoch_ticks), and holds 256
pieces (LDS of its own behind the stage).  The product looks at the clock at the end of every line; builds with
-DBVCF_EXP_PEND_LOOK=n also look after every n-th chunk inside a line, so that a flush can come between two chunks, with
a list or a map of that line in the making -- the cases are written for both (the figures in
profiles/k_stream_store_windows.txt come from such builds).  Results are where they always were: every case is the
streaming path through the library against the oracle, byte for byte.

No case can place a flush by the wall clock, so each runs three times: BVCF_PEND_EPOCH_TICKS unset (the product's epoch),
0 (no clock: the log leaves at capacity, at the pipeline's exits and ahead of direct stores only) and 1 (every look finds
an epoch boundary: a flush at every look).  Nothing here looks at timing.

Pieces per line (see test_gpu_stream_pending.py): entry 2, head bitmap 2 (not on the first line of a pipeline run), a
class list of n entries (n + 4) // 4 (n <= 15), a dense map of 2 504 samples 40 -- a dense line is 44 pieces, a list line
5..8.  The log leaves at a line's end once the largest line of the geometry would no longer fit: above 256 - 44 = 212
pieces at 2 504 samples, above 256 - 8 = 248 at 255."""
import functools
import random

import pytest

import vcfgen
from test_gpu_parity import both
from test_gpu_stream_pending import _same_batch, body_of, row, vcf_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["unset", "0", "1"])
def epoch(request, monkeypatch):
    monkeypatch.setenv("BVCF_PATH", "2")
    monkeypatch.setenv("BVCF_GEN_STREAM", "0")
    if request.param == "unset":
        monkeypatch.delenv("BVCF_PEND_EPOCH_TICKS", raising=False)
    else:
        monkeypatch.setenv("BVCF_PEND_EPOCH_TICKS", request.param)
    return request.param


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


@functools.lru_cache(maxsize=None)
def cached_vcf(ns, ks, seed, alt="G", gts_alt=("0|1", "1|0", "1|1", ".|.")):
    """(the three epoch settings of a case share its bytes)"""
    return vcf_of(ns, list(ks), seed=seed, alt=alt, gts_alt=gts_alt)


# ---- a flush in the middle of a line whose map is in the making

@pytest.mark.parametrize("ns", [2504, 300])
def test_mid_line_flush_with_a_map_in_the_making(bv, ns):
    """dense lines (70, 64, 200 non-reference lanes -- 64 goes from list to stage at its 64th lane, on the way) alternate
    with lists of 0..15 entries: the map appended at the last chunk lands in a log a look has just emptied"""
    lanes = (ns + 3) // 4
    dense = [min(k, lanes) for k in (70, 64, 200)]
    ks = []
    for i in range(16):
        ks += [dense[i % 3], i, dense[(i + 1) % 3], dense[(i + 2) % 3], 15 - i]
    both(bv, cached_vcf(ns, tuple(ks), 100 + ns))


# ---- every chunk count: the looks inside a line come after every n-th chunk, never after its last

@pytest.mark.parametrize("ns", [255, 256, 260, 1030, 2504, 2560])
def test_every_chunk_count(bv, ns):
    """1, 2, 5 and 10 chunks per line; 256 and 2 560 samples take the unaligned loads.  A line of one or two chunks has no
    look inside it"""
    rng = random.Random(ns)
    ks = tuple(rng.choice([0, 1, 4, 15, 16, 40, 64, 200]) for _ in range(120 if ns < 1100 else 60))
    both(bv, cached_vcf(ns, ks, ns + 7, alt="C,G", gts_alt=("0|1", "1|1", ".|.", "1|.", "2|1")))


@pytest.mark.parametrize("n_chunks", [3, 4, 6, 7, 8, 9])
def test_the_chunk_counts_between(bv, n_chunks):
    """the other instantiations of the pipeline: 3..9 chunks, a last chunk that is nearly empty or nearly full"""
    rng = random.Random(n_chunks)
    for ns in (256 * (n_chunks - 1) + 1, 256 * n_chunks - 3):
        ks = tuple(rng.choice([0, 2, 15, 16, 64, 100]) for _ in range(60))
        both(bv, cached_vcf(ns, ks, ns))


# ---- the new capacity, to the piece

@pytest.mark.parametrize("tail", [(0, 1, 2, 3, 13, 14), (0, 1, 2, 5, 13, 14), (0, 1, 2, 3, 0, 1, 2), (12,), ()])
def test_exactly_at_capacity(bv, tail):
    """2 504 samples: the log leaves once more than 212 pieces wait.  Four dense lines are 176 pieces (174 when the first
    opens the pipeline run); lists of 5 + 5 + 5 + 5 + 8 + 8 = 36 behind them reach 212, 5 + 5 + 5 + 6 + 8 + 8 = 213, seven
    lists of 5 = 211; one list of 8, and none (five dense lines: 220).  The pattern repeats, so that it meets the log at
    every fill it can have -- 211, 212 and 213 among them"""
    seed = 7 * len(tail) + sum(tail)
    both(bv, cached_vcf(2504, tuple(([70, 80, 64, 90] + list(tail)) * 10), seed))
    both(bv, cached_vcf(2504, tuple(([70, 80, 64, 90, 66] + list(tail)) * 8), seed + 1))


def test_log_filled_to_the_last_piece(bv):
    """255 samples: a line is 8 pieces at most (a map of 64 bytes), so the log leaves once more than 248 wait, and lines of
    5..8 pieces (lists of 0..15 entries, maps) fill it to every count up to 256, the last piece included"""
    rng = random.Random(177)
    both(bv, cached_vcf(255, tuple(rng.choice([0, 2, 4, 5, 8, 11, 12, 15, 16, 30]) for _ in range(600)), 178))


# ---- direct stores and exits after a mid-line flush

def test_multiallelic_and_raw_lists(bv):
    """further alleles' lists (few carriers: stored directly, the log flushed ahead of them), a raw list behind the slot
    (16..63 non-reference lanes with carriers of ALT #2, or a dense line with a few of them), between plain lines"""
    rng = random.Random(141)
    ns = 2504
    rows, pos = [vcfgen.header(ns)], 500
    for i in range(120):
        pos += 4
        kind = i % 8
        if kind in (1, 5):
            rows.append(row(rng, ns, pos, rng.choice([2, 9, 14]), alt="G,T,C", gts_alt=("0|1", "2|1", "0|2", "3|3", ".|2")))
        elif kind == 3:
            rows.append(row(rng, ns, pos, rng.choice([16, 40, 63]), alt="G,T", gts_alt=("0|1", "1|1", "0|2", "2|2")))
        elif kind == 6:
            f = row(rng, ns, pos, 120, alt="G,T").rstrip("\n").split("\t")
            for s in rng.sample(range(ns), 5):
                f[9 + s] = rng.choice(["0|2", "2|1", "2|2"])
            rows.append("\t".join(f) + "\n")
        else:
            rows.append(row(rng, ns, pos, rng.choice([0, 1, 6, 15, 70])))
    both(bv, "".join(rows).encode())


@pytest.mark.parametrize("k", [1, 2, 5])
def test_malformed_field_after_a_dense_run(bv, k):
    """a sample field that is no genotype (same length: the line looks regular until it is scanned) k lines after a run
    of dense lines: the pipeline is left with whatever the last look did not take"""
    rng = random.Random(110 + k)
    ns = 2504
    rows, pos = [vcfgen.header(ns)], 100
    for rep in range(10):
        for kk in [70, 66, 90, 200, 64] + [rng.randint(0, 15) for _ in range(k - 1)]:
            pos += 5
            rows.append(row(rng, ns, pos, kk))
        pos += 5
        bad = row(rng, ns, pos, 3).rstrip("\n").split("\t")
        bad[9 + rng.randrange(ns)] = rng.choice(["0|x", "0:1", "|01", "1|:"])
        rows.append("\t".join(bad) + "\n")
    both(bv, "".join(rows).encode(), {"allow": ""})


@functools.lru_cache(maxsize=None)
def _with_gt_dp_lines():
    ns = 2504
    rng = random.Random(121)
    ks = [rng.choice([0, 2, 7, 15, 16, 70]) for _ in range(72)]
    rows = [row(rng, ns, 1000 + 3 * i, k) for i, k in enumerate(ks)]
    # GT:DP lines in between: longer than 4 ns bytes, the predicted line end holds no terminator
    for i in range(5, len(rows), 9):
        f = rows[i].rstrip("\n").split("\t")
        rows[i] = "\t".join(f[:8] + ["GT:DP"] + [g + ":%d" % rng.randint(0, 30) for g in f[9:]]) + "\n"
    return (vcfgen.header(ns) + "".join(rows)).encode()


def test_gt_dp_lines_between_regular_ones(bv):
    both(bv, _with_gt_dp_lines(), {"allow": ""})


@pytest.mark.parametrize("cut", [1, 1 + 4 * 1000, 1 + 10000])
def test_unterminated_last_line(bv, cut):
    """no terminator; cut in the sample region; cut in the head (a line of 2 504 samples is 10 016 + ~40 bytes)"""
    both(bv, _with_gt_dp_lines()[:-cut], {"allow": ""})


# ---- lines crossing tiles

@pytest.mark.parametrize("ns", [300, 1030, 2504])
def test_lines_cross_tiles(bv, monkeypatch, ns):
    monkeypatch.setenv("BVCF_TILE_KB", "4")
    rng = random.Random(131 + ns)
    ks = tuple(rng.choice([0, 1, 3, 8, 15, 16, 70]) for _ in range(200 if ns < 2000 else 120))
    vcf = cached_vcf(ns, ks, ns + 11)
    both(bv, vcf)
    both(bv, vcf, max_batch_bytes=1 << 20)


# ---- batches in flight

def test_two_batches_in_flight_on_three_slots(bv):
    """each batch against the same bytes processed alone, twice over, and against the oracle"""
    rng = random.Random(151)
    ns = 2504
    parts = []
    for seed in (1, 2):
        ks = tuple(rng.choice([0, 1, 3, 8, 15, 16, 63, 70]) for _ in range(120))
        parts.append(cached_vcf(ns, ks, 150 + seed, alt="G,T", gts_alt=("0|1", "1|1", ".|.", "0|2")))
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


# ---- no log at all

def test_seventeen_chunks_store_directly(bv):
    """4 097 samples: more chunks than the pipeline holds, every store direct, whatever the epoch says"""
    rng = random.Random(4097)
    ks = tuple(rng.choice([0, 1, 4, 15, 16, 40, 64, 200]) for _ in range(60))
    both(bv, cached_vcf(4097, ks, 4097, alt="C,G", gts_alt=("0|1", "1|1", ".|.", "1|.", "2|1")))
