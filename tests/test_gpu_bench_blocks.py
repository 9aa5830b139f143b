"""The batches bench.py times, compared with the CPU oracle row for row.

bench.py's headline runs device-resident blocks of bench.SHAPES rows (up to 3.2 GB each) through the ctx of
bench.py:1057-1066 with three blocks in flight.  Here the same blocks go through the same ctx after the same kind of
bench_device warm-up, then through bvcf_submit_device / bvcf_collect -- three submitted before the first collect, then
collects and submits in turn -- and every batch's TSV and log, made by bvcf_format_tsv, must equal the oracle's output for
the block's bytes.  Also: blocks whose shape changes between batches in flight, sites-only batches that outgrow the
collect's host buffers, and the --sampleStats table where k_ss_dense splits the dense rows into runs longer than 64."""
import numpy as np
import pytest

import blockcheck as bc

pytestmark = pytest.mark.gpu

ORC = bc.Oracle()  # (the c3 / c4 blocks go through two device paths: one oracle run each)
N_BLOCKS = 4       # bench.rank_blocks(0, 4, rows): the first four of a step's blocks
KSS_MIN_RUN, KSS_COLS = 64, 5  # bvcf_samplestats.hip.h


@pytest.fixture(scope="module")
def mods():
    import bench
    import benchgen as bg
    import bystro_vcf_amd as bv
    return bench, bg, bv


def bench_ctx(bv, bg, cfg, profile, rows, max_bytes, path=0, golden=False, **kw):
    """the ctx of bench.py:1057-1066 at its default --slots 3, as a plain run makes it (class maps on; sites-only input
    packed).  n_alt_cap and cmap_bytes are bench.py:1059 and :1063"""
    ns = cfg.n_samples
    stride = ((ns + 3) // 4 + 15) & ~15
    n_alt_cap = rows * (4 if profile == "c4" or golden else 2 if profile.startswith("c5") else 1) + 1024
    return bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=max_bytes, n_slots=3, max_lines=rows + 16, max_alleles=n_alt_cap,
                  cmap_bytes=min((n_alt_cap + (max_bytes // (4 * ns + 8) if ns else 0) + 16 * 8192) * stride + 4096, 0xFFFFFF00),
                  path=path, want_class_maps=True, packed_sites=ns == 0, **kw)


def max_runs(stride):
    """k_ss_dense's most runs per batch (bvcf_core.hip: 16 MiB of per-run partial counts)"""
    return min(4096, max(1, (16 << 20) // (4 * KSS_COLS * 4 * stride)))


def in_flight(bv, ctx, blocks, on_batch, kernels=None):
    """blocks: [(tensor, nbytes, key, cfg dict, header)].  Three submitted before the first collect (a fourth is refused:
    every slot is in flight), then a collect and a submit in turn, so block 3 reuses block 0's slot while 1 and 2 are
    still in flight.  Each block is copied to the host right before its collect; on_batch(i, batch, host buffer).
    kernels: the streaming kernel each block was launched with is appended to it"""
    n = len(blocks)
    assert n > 3

    def submit(i):
        if kernels is not None:
            kernels.append(ctx.stream_kernel())
        ctx.submit_device(blocks[i][0].data_ptr(), blocks[i][1], seq=i)

    for i in range(3):
        submit(i)
    with pytest.raises(bv.BvcfError) as e:
        ctx.submit_device(blocks[3][0].data_ptr(), blocks[3][1], seq=3)
    assert e.value.rc == bv.E_BUSY
    nxt = 3
    for i in range(n):
        t, nbytes, key, cfgd, hdr = blocks[i]
        buf, nh = bc.host_copy(t, nbytes, hdr)
        b = ctx.collect(tsv=(bc.block_view(buf, nh), bv.make_config(cfgd, n_format_threads=bc.THREADS), bc.sample_names(hdr)))
        assert b.batch_seq == i
        if nxt < n:
            submit(nxt)
            nxt += 1
        ORC.check(key, buf, cfgd, b.tsv, b.log, "block %d (%s)" % (i, key))
        on_batch(i, b, buf)
        del buf, b


def make_blocks(bench, bg, bv, profile, cfgd, rows=None, n=N_BLOCKS, **over):
    cfg = bg.make_cfg(profile, **over)
    rows = rows or bench.SHAPES[profile][0]
    hdr = bg.header(cfg)
    out = []
    for first in bench.rank_blocks(0, n, rows):
        t, nbytes = bg.rows_device(cfg, first, rows, pad=bv.DEVICE_PAD)
        out.append((t, nbytes, (profile, tuple(sorted(over.items())), first, rows, tuple(sorted(cfgd.items()))), cfgd, hdr))
    return cfg, rows, out


@pytest.mark.parametrize("profile,path", [("c3", 0), ("c3", 1), ("c4", 0), ("c4", 1), ("c5", 0), ("c5h", 0), ("c2", 0), ("c2r", 0)])
def test_bench_blocks_equal_the_oracle(mods, profile, path):
    """bench.SHAPES blocks through bench.py's ctx, three in flight, every row against the oracle; the counts bench_device
    reports for its last step equal those of the same block collected on the same ctx"""
    import torch
    bench, bg, bv = mods
    render = profile == "c2r"
    prof = "c2" if render else profile
    cfgd = {"keepId": True, "keepInfo": True} if prof == "c4" else {}
    cfg, rows, blocks = make_blocks(bench, bg, bv, prof, cfgd)
    sizes = [b[1] for b in blocks]
    ptrs = [b[0].data_ptr() for b in blocks]
    if prof == "c3":
        assert max(sizes) > 1 << 31
    kw = {"render_sites": True, "keep_id": False, "keep_info": False} if render else {}
    ctx = bench_ctx(bv, bg, cfg, prof, rows, max(sizes), path=path, **kw)
    try:
        # bench.py's warm-up: every resident block once (bench_device on the ctx's slots)
        _, _, counts = ctx.bench_device(ptrs, sizes, len(blocks))
        assert counts[0] == rows
        if cfg.n_samples:
            assert ctx.path() == (path or 2)
            assert ctx.stream_kernel() == (None if path == 1 else "k_stream_gen" if prof.startswith("c5") else "k_stream")
        seen = {}

        def on_batch(i, b, buf):
            assert b.n_lines == rows and b.n_lines_seen == rows
            if i == len(blocks) - 1:
                seen["last"] = b
            if render:
                assert b.rendered and len(b.rows) > 0

        in_flight(bv, ctx, blocks, on_batch)
        b = seen["last"]
        # bench_device's counters of its last step (the last block): lines, line + further allele slots, errors
        assert counts[0] == b.n_lines and counts[2] == len(b.errs)
        if not cfg.n_samples:
            assert counts[1] >= counts[0]
        else:
            assert counts[1] == len(b.alleles), (counts, len(b.alleles))
    finally:
        ctx.close()
        del blocks
        torch.cuda.empty_cache()


def test_golden_body_in_one_block_past_2_gib(mods, golden_1kg):
    """bench.py --golden: the 1000-Genomes rows copied into one block of more than 2^31 bytes, through the bench's ctx; the
    batch's TSV is the oracle's output for one copy, repeated"""
    import torch
    bench, bg, bv = mods
    raw = golden_1kg[0]
    cut = raw.index(b"\n", raw.index(b"#CHROM")) + 1
    hdr, body = raw[:cut], raw[cut:]
    n_body = body.count(b"\n")
    reps = max(1, bench.SHAPES["c3"][0] // n_body)  # bench.py:1040-1042
    rows = reps * n_body
    nbytes = len(body) * reps
    assert nbytes > 1 << 31
    rc, want, want_log, n = bc.run_oracle(np.frombuffer(raw, np.uint8))
    assert rc == 0 and n == n_body
    host = np.empty(len(hdr) + nbytes, dtype=np.uint8)
    host[:len(hdr)] = np.frombuffer(hdr, np.uint8)
    host[len(hdr):].reshape(reps, len(body))[:] = np.frombuffer(body, np.uint8)
    t = torch.full((nbytes + bv.DEVICE_PAD,), 10, dtype=torch.uint8, device="cuda")
    t[:nbytes].copy_(torch.from_numpy(host[len(hdr):]))
    cfg = bg.make_cfg("c3")
    ctx = bench_ctx(bv, bg, cfg, "c3", rows, nbytes, golden=True)
    try:
        _, _, counts = ctx.bench_device([t.data_ptr()], [nbytes], 1)
        assert counts[0] == rows
        ctx.submit_device(t.data_ptr(), nbytes)
        b = ctx.collect(tsv=(bc.block_view(host, len(hdr)), bv.make_config({}, n_format_threads=bc.THREADS), bc.sample_names(hdr)))
        assert b.n_lines == rows and counts[1] == len(b.alleles) and counts[2] == len(b.errs)
        if b.tsv != want * reps or b.log != want_log * reps:
            bc.compare(want * reps, want_log * reps, b.tsv, b.log, "golden block")
    finally:
        ctx.close()
        del t
        torch.cuda.empty_cache()


def test_shape_changes_between_batches_in_flight(mods):
    """one ctx over c3 -> c5 -> c4 -> c5h -> c3 blocks, three in flight: the streaming kernel switches between batches
    (the ctx learns the shape from a collected batch) and the k_gt / k_finish grids are sized from an earlier batch"""
    import torch
    bench, bg, bv = mods
    seq = [("c3", 40_000, 1_000_000), ("c5", 16_000, 2_000_000), ("c4", 40_000, 3_000_000), ("c5h", 16_000, 4_000_000),
           ("c3", 40_000, 5_000_000)]
    cfgd = {"keepId": True, "keepInfo": True}
    blocks = []
    hdrs = set()
    for prof, rows, first in seq:
        cfg = bg.make_cfg(prof)
        hdr = bg.header(cfg)
        hdrs.add(hdr)
        t, nbytes = bg.rows_device(cfg, first, rows, pad=bv.DEVICE_PAD)
        blocks.append((t, nbytes, (prof, first, rows, "keep"), cfgd, hdr))
    assert len(hdrs) == 1
    rows = max(r for _, r, _ in seq)
    ctx = bench_ctx(bv, bg, cfg, "c4", rows, max(b[1] for b in blocks))
    kernels = []
    try:
        in_flight(bv, ctx, blocks, lambda i, b, buf: None, kernels)
    finally:
        ctx.close()
        del blocks
        torch.cuda.empty_cache()
    assert kernels[0] == "k_stream" and "k_stream_gen" in kernels, kernels


def test_sites_only_rendered_rows_regrow_between_batches(mods):
    """sites-only blocks with the rows rendered on the device: SNP blocks, then a block whose every line the host formats
    (all indels), then SNPs again -- the collect's host buffers for the lines left to the host grow mid-stream"""
    import torch
    bench, bg, bv = mods
    seq = [({}, 0), ({}, 300_000), ({"p_indel": 10000}, 600_000), ({}, 900_000), ({"p_indel": 10000}, 1_200_000), ({}, 1_500_000)]
    rows = 300_000
    blocks = []
    for over, first in seq:
        cfg = bg.make_cfg("c2", **over)
        t, nbytes = bg.rows_device(cfg, first, rows, pad=bv.DEVICE_PAD)
        blocks.append((t, nbytes, ("c2", tuple(sorted(over.items())), first, rows, "render"), {}, bg.header(cfg)))
    ctx = bench_ctx(bv, bg, bg.make_cfg("c2"), "c4", rows, max(b[1] for b in blocks), render_sites=True)
    cuts = []
    try:
        in_flight(bv, ctx, blocks, lambda i, b, buf: cuts.append(len(b.row_cuts)))
    finally:
        ctx.close()
        del blocks
        torch.cuda.empty_cache()
    assert cuts[2] == cuts[4] == rows and cuts[0] < rows // 100 and cuts[5] < rows // 100, cuts


@pytest.mark.parametrize("profile,rows,n_samples", [("c3d", 40_000, 0), ("c3", 0, 0), ("c3d", 3_000, 40_000)])
def test_sample_stats_past_the_first_regime(mods, profile, rows, n_samples):
    """bvcf_sample_stats over collected batches equals the counts of their class maps (numpy), and the batches' TSV equals
    the oracle's (which pins the maps): every row dense with more than 64 x max_runs dense rows in one batch (k_ss_dense's
    runs longer than 64 rows); two c3 bench blocks in flight; a cohort of 40 000 samples on the path the library picks
    (the census path with k_gt_wide)"""
    import torch
    bench, bg, bv = mods
    over = {"n_samples": n_samples} if n_samples else {}
    n_blocks = 2 if profile == "c3" else 1
    cfg, rows, blocks = make_blocks(bench, bg, bv, profile, {}, rows=rows or None, n=n_blocks, **over)
    ns = cfg.n_samples
    stride = ((ns + 3) // 4 + 15) & ~15
    n_alt = rows + 1024
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=max(b[1] for b in blocks), n_slots=3, max_lines=rows + 16,
                 max_alleles=n_alt, cmap_bytes=min((n_alt + 16 * 8192) * stride + 4096, 0xFFFFFF00), sample_stats=True)
    want = np.zeros((ns, 6), dtype=np.uint64)
    dense = []
    try:
        assert ctx.path() == (1 if ns >= 32768 else 2)
        for i, (t, nbytes, key, cfgd, hdr) in enumerate(blocks):
            ctx.submit_device(t.data_ptr(), nbytes, seq=i)
        for i, (t, nbytes, key, cfgd, hdr) in enumerate(blocks):
            buf, nh = bc.host_copy(t, nbytes, hdr)
            b = ctx.collect(tsv=(bc.block_view(buf, nh), bv.make_config({}, n_format_threads=bc.THREADS), bc.sample_names(hdr)))
            ORC.check(key, buf, {}, b.tsv, b.log, "block %d (%s)" % (i, key))
            del buf
            slots, mapped = bc.row_records(b)
            dense.append(int((mapped & ((b.alleles["flags"][slots] & 2) == 0)).sum()))
            want += bc.expected_sample_counts(b)
            del b
        got = ctx.sample_stats()
    finally:
        ctx.close()
        del blocks
        torch.cuda.empty_cache()
    if profile == "c3d":
        assert dense[0] > KSS_MIN_RUN * max_runs(stride), (dense, max_runs(stride))
    assert got.shape == want.shape and want[:, 5].min() > 0
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), "samples %s: got %s want %s" % (bad[:5].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())
