"""The bench's synthetic row model: device generator == host generator, and HIP path == oracle on it
(BASELINE configs 1-3 shapes at sizes the oracle finishes in seconds)."""
import numpy as np
import pytest

import blockcheck as bc
import oracle_lib as orc

pytestmark = pytest.mark.gpu

ORC = bc.Oracle()  # (each full-size block goes through several device paths: one oracle run)


def collect_checked(bv, ctx, t, nbytes, hdr, key, cfgd=None):
    """ctx.collect() of the block in t, with the whole batch's TSV and log compared with the oracle's"""
    buf, nh = bc.host_copy(t, nbytes, hdr)
    b = ctx.collect(tsv=(bc.block_view(buf, nh), bv.make_config(cfgd, n_format_threads=bc.THREADS), bc.sample_names(hdr)))
    ORC.check(key, buf, cfgd, b.tsv, b.log, "block %r" % (key,))
    return b


@pytest.fixture(autouse=True, params=["census", "streaming", "census-wide", "streaming-general"])
def bvcf_path(request, monkeypatch):
    """every parity test runs on both device paths (bvcf_params.path; BVCF_PATH overrides `choose`), on the census
    path with the regular scan split over waves as it is for cohorts of >= 32 768 samples (k_gt_wide), and on the
    streaming path with k_stream_gen pinned (see test_gpu_parity.py)"""
    monkeypatch.setenv("BVCF_PATH", "2" if request.param.startswith("streaming") else "1")
    monkeypatch.setenv("BVCF_GEN_STREAM", "1" if request.param == "streaming-general" else "0")
    if request.param == "census-wide":
        monkeypatch.setenv("BVCF_WIDE", "1")
        monkeypatch.setenv("BVCF_WIDE_WIN", "1000")  # the general scan of one line in 1000-byte shares
    return request.param


@pytest.fixture(scope="module")
def mods():
    import benchgen as bg
    import bystro_vcf_amd as bv
    return bg, bv


@pytest.mark.parametrize("profile,first,n", [("c2", 0, 5000), ("c3", 123456, 600), ("c4", 999, 600), ("c5", 77, 400), ("c5h", 77, 400)])
def test_device_rows_equal_host_rows(mods, profile, first, n):
    bg, bv = mods
    cfg = bg.make_cfg(profile)
    host = bg.rows_host(cfg, first, n)
    t, nbytes = bg.rows_device(cfg, first, n)
    assert nbytes == len(host)
    assert bytes(t[:nbytes].cpu().numpy()) == host


@pytest.mark.parametrize("profile,n,cfgd", [
    ("c2", 20000, {}),
    ("c3", 3000, {}),
    ("c4", 3000, {"keepId": True, "keepInfo": True}),
    ("c5", 2000, {}),
    ("c5h", 2000, {}),
])
def test_parity_on_bench_shapes(mods, profile, n, cfgd):
    bg, bv = mods
    cfg = bg.make_cfg(profile)
    vcf = bg.header(cfg) + bg.rows_host(cfg, 5_000_000, n)
    rc_o, out_o, log_o, n_o = orc.run(vcf, cfgd, n_threads=8)
    rc_g, out_g, log_g, n_g = bv.run_buffer(vcf, cfgd, max_batch_bytes=8 << 20)
    assert rc_o == 0 and rc_g == 0 and n_o == n_g == n
    assert out_g == out_o
    assert log_g == log_o
    if profile == "c4":
        assert log_g.count("\n") > 0 and out_g.count(b"MULTIALLELIC") > 0 and out_g.count(b"\tDEL\t") > 0


def test_full_size_properties_c3(mods):
    """BASELINE-size batch (131 072 rows x 2 504 samples, 1.33 GB) through the device-resident entry: the whole batch's
    TSV against the oracle, and size-independent properties: every row is a passing biallelic SNP,
    an == 2*ns, ac == n_het + 2*n_hom, ac > 0, and two passes give identical counters."""
    import torch
    bg, bv = mods
    cfg = bg.make_cfg("c3")
    rows = 131072
    t, nbytes = bg.rows_device(cfg, 777_000_000, rows, pad=bv.DEVICE_PAD)
    stride = ((cfg.n_samples + 3) // 4 + 15) & ~15
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, n_slots=1, max_lines=rows + 16,
                 max_alleles=rows + 1024, cmap_bytes=(rows + 1024 + 16 * 8192) * stride)
    ctx.submit_device(t.data_ptr(), nbytes)
    b = collect_checked(bv, ctx, t, nbytes, bg.header(cfg), ("c3", 777_000_000, rows))
    assert len(b.lines) == rows and (b.lines["status"] == bv.LINE_OK).all()
    assert (b.lines["n_rec"] == 1).all() and (b.lines["n_fields"] == bg.n_header_fields(cfg)).all()
    al = b.alleles[:rows]
    assert (al["an"] == 2 * cfg.n_samples).all() and (al["n_miss"] == 0).all()
    assert (al["ac"] == al["n_het"] + 2 * al["n_hom"]).all() and (al["ac"] > 0).all()
    # class maps agree with the counters on a sample of rows
    for i in np.linspace(0, rows - 1, 50).astype(int):
        cls = b.classes(al[i])
        assert (cls == 1).sum() == al["n_het"][i] and (cls == 2).sum() == al["n_hom"][i]
    # spot-check rows against the oracle
    host = bytes(t[:nbytes].cpu().numpy())
    lines = host.split(b"\n")
    hdr = bg.header(cfg)
    pick = [0, 1, rows // 2, rows - 1]
    rc, out, _, _ = orc.run(hdr + b"".join(lines[i] + b"\n" for i in pick))
    orows = [r.split(b"\t") for r in out.split(b"\n") if r]
    for i, r in zip(pick, orows):
        assert int(r[12]) == al["ac"][i] and int(r[13]) == al["an"][i]
    ctx.submit_device(t.data_ptr(), nbytes)
    b2 = ctx.collect()
    assert (b2.alleles[:rows]["ac"] == al["ac"]).all()
    ctx.close()


def test_full_size_properties_c4(mods):
    """BASELINE configs[3] at bench size (65 536 rows x 2 504 samples, 20 % multiallelic, 15 % indels,
    1 % malformed): the whole batch's TSV and log against the oracle, invariants that hold for every record whatever the
    data, and oracle spot checks."""
    import torch
    bg, bv = mods
    cfg = bg.make_cfg("c4")
    rows = 65536
    ns = cfg.n_samples
    t, nbytes = bg.rows_device(cfg, 42_000_000, rows, pad=bv.DEVICE_PAD)
    stride = ((ns + 3) // 4 + 15) & ~15
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, n_slots=1, max_lines=rows + 16,
                 max_alleles=4 * rows, cmap_bytes=(4 * rows + 16 * 8192) * stride)
    ctx.submit_device(t.data_ptr(), nbytes)
    b = collect_checked(bv, ctx, t, nbytes, bg.header(cfg), ("c4", 42_000_000, rows, "keep"), {"keepId": True, "keepInfo": True})
    ctx.close()
    assert len(b.lines) == rows and b.n_lines_seen == rows
    ok = b.lines["status"] == bv.LINE_OK
    assert 0.97 * rows < ok.sum() < rows            # ~1 % malformed rows yield no allele
    assert (b.lines["status"][~ok] == bv.LINE_NOALLELE).all()
    n_multi = n_del = n_ins = 0
    for i in np.flatnonzero(ok)[:: 37]:
        recs = b.records(int(i))
        assert len(recs) == b.lines["n_rec"][i] >= 1
        for r in recs:
            assert r["an"] == 2 * ns and r["n_miss"] == 0
            assert r["ac"] == r["n_het"] + 2 * r["n_hom"]
            cls = b.classes(r)
            assert (cls == 1).sum() == r["n_het"] and (cls == 2).sum() == r["n_hom"] and (cls == 3).sum() == 0
        n_multi += recs[0]["site_type"] == 4
        n_del += recs[0]["site_type"] == 2
        n_ins += recs[0]["site_type"] == 1
        if recs[0]["site_type"] == 4:               # alleles of one site partition the carriers
            assert sum(int(r["ac"]) for r in recs) <= 2 * ns
    assert n_multi > 100 and n_del > 30 and n_ins > 30
    # oracle on a sample of whole lines
    host = bytes(t[:nbytes].cpu().numpy())
    lines = host.split(b"\n")
    pick = list(range(0, rows, 1499))
    rc, out, _, _ = orc.run(bg.header(cfg) + b"".join(lines[i] + b"\n" for i in pick), {"keepInfo": True})
    want = {}
    for r in out.split(b"\n"):
        if r:
            f = r.split(b"\t")
            want.setdefault(f[-1], []).append((f[1], f[4], int(f[12]), int(f[13]), int(f[-2])))
    for i in pick:
        L = b.lines[i]
        info = lines[i].split(b"\t")[7]
        got = [(r["ac"], r["an"], r["alt_idx"]) for r in b.records(i) if r["ac"] > 0]
        assert sorted((a, n, k) for (_, _, a, n, k) in want.get(info, [])) == sorted((int(a), int(n), int(k)) for a, n, k in got)


def test_block_past_2_gib(mods, bvcf_path):
    """one block of 311 296 rows (3.16 GB, bench.py's block): byte offsets above 2^31 -- the line index, the head
    windows and the scans compare offsets as unsigned 32-bit values, a signed difference would wrap there.  The whole
    batch's TSV against the oracle, size-independent properties over every row, and oracle spot checks on rows from both
    sides of the 2 GiB mark."""
    if bvcf_path == "census-wide":
        pytest.skip("same kernels as census at this sample count")
    bg, bv = mods
    cfg = bg.make_cfg("c3")
    rows = 311_296
    t, nbytes = bg.rows_device(cfg, 31_000_000, rows, pad=bv.DEVICE_PAD)
    assert nbytes > (1 << 31) + (1 << 29)
    stride = ((cfg.n_samples + 3) // 4 + 15) & ~15
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, n_slots=1, max_lines=rows + 16,
                 max_alleles=rows + 1024, cmap_bytes=(rows + 1024 + 16 * 8192) * stride)
    ctx.submit_device(t.data_ptr(), nbytes)
    b = collect_checked(bv, ctx, t, nbytes, bg.header(cfg), ("c3", 31_000_000, rows))
    ctx.close()
    assert len(b.lines) == rows and b.n_lines_seen == rows and (b.lines["status"] == bv.LINE_OK).all()
    off = b.lines["off"].astype(np.int64)
    ln = b.lines["len"].astype(np.int64)
    assert off[0] == 0 and (off[1:] == off[:-1] + ln[:-1] + 1).all() and off[-1] + ln[-1] + 1 == nbytes
    assert (b.lines["n_fields"] == bg.n_header_fields(cfg)).all() and (b.lines["n_rec"] == 1).all()
    al = b.alleles[:rows]
    assert (al["an"] == 2 * cfg.n_samples).all() and (al["n_miss"] == 0).all()
    assert (al["ac"] == al["n_het"] + 2 * al["n_hom"]).all() and (al["ac"] > 0).all()
    pick = [0, rows // 3, int(np.searchsorted(off, 1 << 31)) - 1, int(np.searchsorted(off, 1 << 31)), rows - 1]
    text = b"".join(bytes(t[int(off[i]):int(off[i] + ln[i] + 1)].cpu().numpy()) for i in pick)
    rc, out, _, _ = orc.run(bg.header(cfg) + text)
    orows = [r.split(b"\t") for r in out.split(b"\n") if r]
    assert len(orows) == len(pick)
    for i, r in zip(pick, orows):
        assert int(r[12]) == al["ac"][i] and int(r[13]) == al["an"][i] and int(r[1]) >= 0
        cls = b.classes(al[i])
        assert (cls == 1).sum() == al["n_het"][i] and (cls == 2).sum() == al["n_hom"][i]
