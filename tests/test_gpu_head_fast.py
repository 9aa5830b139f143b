"""k_order's fast lane on the device: with BVCF_HEAD_FAST=1 (the default) plain SNP lines are settled by k_order and
k_head walks the list of the others; with BVCF_HEAD_FAST=0 every line is listed.  Either way, on ctxs of one slot (k_head)
and of three (k_head_lean), the TSV and the log are the oracle's, and lines[] / alleles[] are the same record by record
(without the layout fields bench.py --dump-outputs leaves out)."""
import numpy as np
import pytest

import blockcheck as bc
import headfast_cases as hc
import oracle_lib as orc

pytestmark = pytest.mark.gpu

LINE_COLS = ("status", "site_type", "n_rec", "n_fields", "off", "len", "fend")
REC_COLS = ("pos", "alt_idx", "alt_off", "alt_len", "ac", "an", "n_het", "n_hom", "n_miss", "ref", "alt_base", "kind",
            "site_type", "trtv")
TILE = 64 << 10  # bvcf_ctx.tile_bytes


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def n_header_of(hdr):
    return [ln for ln in hdr.split(b"\n") if ln.startswith(b"#CHROM")][0].rstrip(b"\r").count(b"\t") + 1


def through(bv, monkeypatch, hdr, body, cfgd, slots, fast, retry=False, **kw):
    """the block through a streaming ctx of `slots` slots with the fast lane on or off -> (Batch with .tsv / .log, lines left
    to k_head, the per-sample table or None)"""
    monkeypatch.setenv("BVCF_HEAD_FAST", "1" if fast else "0")
    cfgd = dict(cfgd or {})
    ctx = bv.Ctx(n_header_of(hdr), allow=cfgd.get("allow", "PASS,."), exclude=cfgd.get("exclude", ""), n_slots=slots, path=2,
                 max_batch_bytes=max(len(body), 1 << 20), **kw)
    try:
        assert ctx.path() == 2
        tsv = (body, bv.make_config(cfgd), bc.sample_names(hdr))
        ctx.submit(body)
        if retry:
            with pytest.raises(bv.BvcfError) as ei:
                ctx.collect()
            assert ei.value.rc == bv.E_CAPACITY
            n = body.count(b"\n")
            ctx.reserve(n + 64, 4 * n + 1024, (2 * n + 4096) * 1024)
            ctx.submit(body)
        b = ctx.collect(tsv=tsv)
        table = ctx.sample_stats() if kw.get("sample_stats") else None
        return b, ctx.head_left(), table
    finally:
        ctx.close()


def same_records(a, b, what):
    assert a.n_lines == b.n_lines and len(a.errs) == len(b.errs), what
    for k in LINE_COLS:
        assert (a.lines[k] == b.lines[k]).all(), (what, k, np.flatnonzero((a.lines[k] != b.lines[k]).reshape(a.n_lines, -1).any(axis=1))[:8])
    has = np.flatnonzero(a.lines["n_rec"] >= 1)
    for k in REC_COLS + ("flags",):
        x, y = a.alleles[k][has], b.alleles[k][has]
        if k == "flags":
            x, y = x & 1, y & 1
        assert (x == y).all(), (what, k, has[np.flatnonzero(x != y)[:8]])
    for i in np.flatnonzero(a.lines["n_rec"] > 1):
        ra, rb = a.records(int(i)), b.records(int(i))
        for k in REC_COLS:
            assert (ra[k] == rb[k]).all(), (what, int(i), k)
    if a.n_samples and len(a.cmap):
        for i in has[:: max(1, len(has) // 200)]:
            ra, rb = a.alleles[int(i)], b.alleles[int(i)]
            assert (int(ra["cmap_off"]) == bv_no_cmap()) == (int(rb["cmap_off"]) == bv_no_cmap())
            if int(ra["cmap_off"]) != bv_no_cmap():
                assert (a.classes(ra) == b.classes(rb)).all(), (what, int(i))
    ea, eb = np.sort(a.errs, order=["line", "alt_no", "code"]), np.sort(b.errs, order=["line", "alt_no", "code"])
    for k in ("line", "alt_no", "code"):
        assert (ea[k] == eb[k]).all(), (what, k)
    if a.dosage is not None:
        for i in has[:: max(1, len(has) // 500)]:
            sa, sb = a.record_slots(int(i)), b.record_slots(int(i))
            assert (a.dosage[sa, :a.n_samples] == b.dosage[sb, :a.n_samples]).all(), (what, int(i))


def bv_no_cmap():
    import bystro_vcf_amd as b
    return b.NO_CMAP


def both_settings(bv, monkeypatch, hdr, body, cfgd, what, want=None, retry=False, **kw):
    """slots 1 and 3, fast lane on and off: each equals the oracle, and on equals off -> {(slots, fast): (batch, left, table)}"""
    if want is None:
        rc, out, log, _ = orc.run(hdr + body, cfgd)
        assert rc == 0
        want = (out, log)
    got = {}
    for slots in (1, 3):
        for fast in (1, 0):
            b, left, table = through(bv, monkeypatch, hdr, body, cfgd, slots, fast, retry=retry, **kw)
            bc.compare(want[0], want[1], b.tsv, b.log, "%s, %d slot(s), BVCF_HEAD_FAST=%d" % (what, slots, fast), cfgd)
            got[(slots, fast)] = (b, left, table)
            if not fast:
                assert left == b.n_lines, "fast lane off: every line is listed"
        same_records(got[(slots, 1)][0], got[(slots, 0)][0], "%s, %d slot(s)" % (what, slots))
        if kw.get("sample_stats"):
            assert (got[(slots, 1)][2] == got[(slots, 0)][2]).all()
            assert (got[(slots, 1)][2] == bc.expected_sample_counts(got[(slots, 1)][0])).all()
    return got


GROUPS = hc.groups()


@pytest.mark.parametrize("key", list(GROUPS), ids=["allow=%s,exclude=%s" % k for k in GROUPS])
def test_crafted_lines(bv, monkeypatch, key):
    cases = GROUPS[key]
    cfgd = {"allow": key[0], "exclude": key[1]}
    hdr, body = hc.header(), hc.body(cases)
    got = both_settings(bv, monkeypatch, hdr, body, cfgd, "crafted lines")
    # the lane agrees with its host twin line by line: what the host entry settles from the model of k_stream's entry is
    # what the device left out of k_head's list, and every ls & 3 occurs among the settled lines
    b, left, _ = got[(3, 1)]
    settled, residues = 0, set()
    for i in range(b.n_lines):
        L = b.lines[i]
        ls, n = int(L["off"]), int(L["len"])
        bits = hc.tab_bits(body, ls)
        first_of_run = i == 0 or ls // TILE != int(b.lines[i - 1]["off"]) // TILE
        if bits is None or first_of_run:
            continue
        v, hl, ha = bv.head_fast_line(body[ls:ls + 80], ls, n | bv.HAS_HEAD_BITS, [0] * 5, bv.NO_CMAP, bits, i, hc.N_HEADER, key[0], key[1])
        if v != bv.HEAD_FAST_DECLINE:
            settled += 1
            residues.add(ls & 3)
            assert int(L["status"]) == int(hl["status"]) and L["fend"].tolist() == hl["fend"].tolist()
    # (lines that are not of the 4-byte grid never carry a bitmap; the crafted lines all are)
    assert left == b.n_lines - settled, (left, b.n_lines, settled)
    if len(cases) > 8:
        assert residues == {0, 1, 2, 3}


@pytest.mark.parametrize("extra", [{"want_dosage": True}, {"sample_stats": True}], ids=["dosageOutput", "sampleStats"])
def test_crafted_lines_with_dosage_and_sample_stats(bv, monkeypatch, extra):
    key = ("PASS,.", "")
    both_settings(bv, monkeypatch, hc.header(), hc.body(GROUPS[key]), {"allow": key[0], "exclude": key[1]}, "crafted lines", **extra)


def test_crlf_takes_no_fast_lane(bv, monkeypatch):
    key = ("PASS,.", "")
    hdr = hc.header().replace(b"\n", b"\r\n")
    body = hc.body(GROUPS[key]).replace(b"\n", b"\r\n")
    got = both_settings(bv, monkeypatch, hdr, body, {"allow": key[0], "exclude": key[1]}, "CRLF", eol_chars=2)
    b, left, _ = got[(3, 1)]
    assert left == b.n_lines  # k_stream's pipeline (the bitmaps) is for one-byte terminators


def test_overflow_and_retry(bv, monkeypatch):
    key = ("PASS,.", "")
    both_settings(bv, monkeypatch, hc.header(), hc.body(GROUPS[key]), {"allow": key[0], "exclude": key[1]}, "retried batch",
                  retry=True, max_lines=16, max_alleles=16, cmap_bytes=4096)


@pytest.mark.parametrize("profile", ["c3", "c4"])
@pytest.mark.parametrize("extra", [{}, {"want_dosage": True}, {"sample_stats": True}], ids=["plain", "dosageOutput", "sampleStats"])
def test_bench_row_models(bv, monkeypatch, profile, extra):
    """bench.py's c3 (biallelic SNPs) and c4 (a fifth multiallelic, indels) rows, 2 504 samples"""
    import benchgen as bg
    cfgd = {"keepId": True, "keepInfo": True} if profile == "c4" else {}
    cfg = bg.make_cfg(profile)
    rows = 1500
    hdr = bg.header(cfg)
    t, nbytes = bg.rows_device(cfg, 0, rows, pad=bv.DEVICE_PAD)
    body = bytes(t[:nbytes].cpu().numpy())
    del t
    got = both_settings(bv, monkeypatch, hdr, body, cfgd, profile + " rows", **extra)
    b, left, _ = got[(3, 1)]
    assert b.n_lines == rows
    if profile == "c3" and not extra:
        # the counter: every line of these rows is a plain SNP, so what is left are the lines without a bitmap -- the first
        # line of each k_stream wave's run.  With fewer tiles than waves a run is one tile.
        assert (nbytes + TILE - 1) // TILE <= 256
        no_bitmap = len(set((b.lines["off"] // TILE).tolist()))
        assert left == no_bitmap, (left, no_bitmap)
        assert got[(1, 1)][1] == no_bitmap
    if profile == "c4":
        assert 0 < left < rows


def test_golden_1kg(bv, monkeypatch, golden_1kg):
    vcf, want_sorted, _ = golden_1kg
    at = vcf.index(b"#CHROM")
    at = vcf.index(b"\n", at) + 1
    hdr, body = vcf[:at], vcf[at:]
    got = {}
    for slots in (1, 3):
        for fast in (1, 0):
            b, left, _ = through(bv, monkeypatch, hdr, body, {}, slots, fast)
            got[(slots, fast)] = b
            if fast:
                assert sorted(b.tsv.split(b"\n")[:-1]) == want_sorted
                assert 0 < left < b.n_lines // 2
        same_records(got[(slots, 1)], got[(slots, 0)], "golden, %d slot(s)" % slots)
        assert got[(slots, 1)].tsv == got[(slots, 0)].tsv and got[(slots, 1)].log == got[(slots, 0)].log
        del got[(slots, 0)]
