"""The byte-parallel decoders over their closed domains (closed_domains.py): every three-byte genotype field the frame mask
can let through, every short general field, every REF / ALT token / POS shape up to the sizes where a decision changes --
each on every device chain that decodes it, against the oracle: TSV bytes, log and line count identical.

What a green run says is "there is no such input below this size", not "we sampled it": a constant of alphabet_bad, one
suffix length of eval_words or the tenth digit of row_atoi9 matters for a handful of these inputs, and each of them is here.

test_closed_domains_cpu.py shows with the oracle alone that the inputs hold what is claimed of them."""
import ctypes as C
import functools

import numpy as np
import pytest

import closed_domains as cd
import gtmask
import oracle_lib as orc
import samplecut

pytestmark = pytest.mark.gpu

CHAINS = {"census": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0"},
          "streaming": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "0"},
          "census-wide": {"BVCF_PATH": "1", "BVCF_GEN_STREAM": "0", "BVCF_WIDE": "1", "BVCF_WIDE_WIN": "1000"},
          "streaming-general": {"BVCF_PATH": "2", "BVCF_GEN_STREAM": "1"}}
GT_PIECES = ["g3-list", "g3-dense", "g3_last-lf", "g3_last-crlf", "g3_2600-list", "g3_2600-raw", "g3_2600-dense",
             "g3_2500-list", "g3_2500-raw", "g3_2500-dense", "gg-gt", "gg-gtdpgq", "gg-gt-last", "gg-gtdpgq-last"]
# (the dosage rows of 2 048 lines x 2 500 samples take the oracle and numpy five seconds to spell out and read back: those
# pieces run as dosage rows in four runs of 512 lines each)
DOSAGE_PARTS = 4
DOSAGE_PIECES = [q for p in GT_PIECES
                 for q in ([p] if not p.startswith("g3_2") else ["%s-part%dof%d" % (p, k, DOSAGE_PARTS) for k in range(DOSAGE_PARTS)])]
CUT_SAMPLE = 6  # neither a probe (samples 8..) nor a carrier (samples 0..5); in the dense lines a non-reference sample
KEEP_ALL = {"keepId": True, "keepInfo": True, "keepPos": True}


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def force(monkeypatch, chain):
    for k in ("BVCF_WIDE", "BVCF_WIDE_WIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in CHAINS[chain].items():
        monkeypatch.setenv(k, v)


@pytest.fixture(params=list(CHAINS))
def chain(request, monkeypatch):
    force(monkeypatch, request.param)
    return request.param


def frozen(cfg):
    return tuple(sorted((cfg or {}).items()))


@functools.lru_cache(maxsize=None)
def oracle(name, cfg=(), gq=0, dp=0, cut=None):
    """(rc, TSV body, log, n lines) of the oracle over a piece -- masked as --minGQ / --minDP would (gtmask), without sample
    `cut` (samplecut) --, computed once"""
    vcf = cd.piece(name)
    if gq or dp:
        vcf = gtmask.mask_vcf(vcf, gq, dp)
    if cut is not None:
        vcf = samplecut.cut_vcf(vcf, kept_without(name, cut))
    res = orc.run(vcf, dict(cfg))
    assert res[0] == 0
    return res


def n_samples_of(name):
    return len(samplecut.sample_names(cd.piece(name)[:40000]))


def kept_without(name, cut):
    return [s for s in range(n_samples_of(name)) if s != cut]


def explain(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (x, y) in enumerate(zip(g, w)):
        if x != y:
            return "row %d differs:\noracle: %r\nhip:    %r" % (i, y[:400], x[:400])
    return "the first %d rows agree; oracle has %d, hip %d" % (min(len(g), len(w)) - 1, len(w) - 1, len(g) - 1)


def hold(bv, vcf, want, cfg=None, **kw):
    """run_buffer of `vcf` against an oracle result: TSV bytes, log and line count identical"""
    rc_o, out_o, log_o, n_o = want
    rc, out, log, n = bv.run_buffer(vcf, cfg, **kw)
    assert rc == 0 and rc_o == 0, (rc, rc_o, log[-300:])
    assert n == n_o
    assert out == out_o, explain(out, out_o)
    assert log == log_o, explain(log.encode(), log_o.encode())


# ------------------------------------------------------------------ G3 and GG through run_buffer

@pytest.mark.parametrize("name", GT_PIECES)
def test_genotype_fields_on_every_chain(bv, chain, name):
    hold(bv, cd.piece(name), oracle(name))


def thresholds_of(name):
    """FORMAT GT: no line names GQ or DP, a threshold masks nothing.  GT:DP:GQ with :5:6 behind every field: 6 / 5 mask only
    the probes whose own colons move other values under the keys, 20 / 10 mask every sample"""
    return [(6, 5), (20, 10)] if "gtdpgq" in name else [(20, 10)]


@pytest.fixture(params=["census", "streaming"])
def base_chain(request, monkeypatch):
    """the chain a ctx would be on without a threshold or a selection (with one it takes the census chain's masked / subset
    scan whatever is forced here: both settings must give the one answer)"""
    force(monkeypatch, request.param)
    return request.param


@pytest.mark.parametrize("name", GT_PIECES)
def test_genotype_fields_on_the_masked_chain(bv, base_chain, name):
    for gq, dp in thresholds_of(name):
        want = oracle(name, (), gq, dp) if "gtdpgq" in name else oracle(name)
        hold(bv, cd.piece(name), want, {"minGQ": gq, "minDP": dp})
    if "gtdpgq" in name:  # (the mask bites: the probes that 6 / 5 mask change rows)
        assert oracle(name, (), 6, 5)[1] != oracle(name)[1] != oracle(name, (), 20, 10)[1]


@pytest.mark.parametrize("name", GT_PIECES)
def test_genotype_fields_on_the_subset_chain(bv, base_chain, tmp_path, name):
    vcf = cd.piece(name)
    keep = samplecut.list_file(tmp_path / "keep.list", vcf[:40000], kept_without(name, CUT_SAMPLE))
    hold(bv, vcf, oracle(name, (), 0, 0, CUT_SAMPLE), {"keepSamples": keep})
    if name in ("g3-dense", "g3_2600-dense", "g3_2500-dense"):  # (the cut bites where the cut sample is not the reference genotype)
        assert oracle(name, (), 0, 0, CUT_SAMPLE)[1] != oracle(name)[1]


# ------------------------------------------------------------------ ... and as dosage rows through a ctx

@functools.lru_cache(maxsize=None)
def oracle_dosage(name, gq=0, dp=0, cut=None):
    """orc.run_dosage's rows as one int8 matrix (rows x samples).  (The call of oracle_lib.run_dosage restated, to keep in step
    with it: that one turns every value into a Python int, seconds per piece at 2 500 samples; here the text is read by numpy.)"""
    vcf = cd.piece(name)
    if gq or dp:
        vcf = gtmask.mask_vcf(vcf, gq, dp)
    if cut is not None:
        vcf = samplecut.cut_vcf(vcf, kept_without(name, cut))
    L = orc.lib()
    L.orc_run_dosage.argtypes = [C.POINTER(orc.OrcConfig), C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.orc_run_dosage.restype = C.c_int
    c = orc.make_config({}, 1)
    out, n_out = C.c_void_p(), C.c_size_t()
    rc = L.orc_run_dosage(C.byref(c), vcf, len(vcf), C.byref(out), C.byref(n_out))
    text = C.string_at(out, n_out.value)
    L.orc_free(out)
    assert rc == 0
    rows = text.split(b"\n")[:-1]
    flat = np.fromstring(b",".join(r.partition(b"\t")[2] for r in rows).decode(), dtype=np.int64, sep=",")
    return flat.astype(np.int8).reshape(len(rows), -1)


def body_of(vcf):
    """(n header fields, CRLF?, the data lines)"""
    hdr_at = vcf.index(b"#CHROM")
    hdr_end = vcf.index(b"\n", hdr_at)
    crlf = vcf[hdr_end - 1:hdr_end] == b"\r"
    return vcf[hdr_at:hdr_end].rstrip(b"\r").count(b"\t") + 1, crlf, vcf[hdr_end + 1:]


def roomy_ctx(bv, n_header, body, n_alts, **kw):
    """a ctx that takes `body` as one batch, with room for a record and a class-map slot (and a raw list) per ALT of every line"""
    n = body.count(b"\n")
    ctx = bv.Ctx(n_header, max_batch_bytes=max(len(body), 1 << 20), **kw)
    stride = ((max(n_header - 9, 0) + 3) // 4 + 15) & ~15
    ctx.reserve(n + 64, (n_alts + 2) * n + 1024, ((n_alts + 8) * n + 4096) * max(stride, 16))
    return ctx


def device_dosage(bv, vcf, n_alts, **kw):
    """the int8 rows bvcf_collect returns for the output alleles of `vcf`, in input order, as a matrix"""
    n_header, crlf, body = body_of(vcf)
    ctx = roomy_ctx(bv, n_header, body, n_alts, want_dosage=True, eol_chars=2 if crlf else 1, **kw)
    try:
        b = ctx.process(body)
    finally:
        ctx.close()
    slots = []
    for i in np.flatnonzero((b.lines["status"] == 0) & (b.lines["n_rec"] > 0)):
        slots += b.record_slots(int(i))
    slots = np.array(slots, dtype=np.int64)
    slots = slots[b.alleles["ac"][slots] != 0]  # main.go:558-560
    return b.dosage[slots, :b.n_samples]


@pytest.mark.parametrize("mode", ["plain", "masked", "subset"])
@pytest.mark.parametrize("path", ["census", "streaming"])
@pytest.mark.parametrize("name", DOSAGE_PIECES)
def test_genotype_fields_as_dosage_rows(bv, monkeypatch, name, path, mode):
    force(monkeypatch, path)
    vcf = cd.piece(name)
    n_alts = 11 if name.startswith("gg") else 9
    if mode == "plain":
        runs = [(oracle_dosage(name), {})]
    elif mode == "masked":
        runs = [(oracle_dosage(name, gq, dp) if "gtdpgq" in name else oracle_dosage(name), {"min_gq": gq, "min_dp": dp})
                for gq, dp in thresholds_of(name)]
    else:
        runs = [(oracle_dosage(name, 0, 0, CUT_SAMPLE), {"sample_keep": kept_without(name, CUT_SAMPLE)})]
    for want, kw in runs:
        got = device_dosage(bv, vcf, n_alts, **kw)
        assert got.shape == want.shape, (got.shape, want.shape)
        if not (got == want).all():
            r, s = np.argwhere(got != want)[0]
            raise AssertionError("dosage row %d differs first at sample %d: oracle %d, hip %d" % (r, s, want[r, s], got[r, s]))


# ------------------------------------------------------------------ the forms the regular scan leaves (streaming chain)

def records_of(bv, monkeypatch, vcf, n_alts=9):
    force(monkeypatch, "streaming")
    n_header, crlf, body = body_of(vcf)
    ctx = roomy_ctx(bv, n_header, body, n_alts)
    try:
        assert ctx.path() == 2
        return ctx.process(body), body
    finally:
        ctx.close()


def sparse_first_records(b):
    ok = np.flatnonzero((b.lines["status"] == 0) & (b.lines["n_rec"] > 0))
    first = b.alleles[ok]
    assert (first["alt_idx"] == 0).all() and len(ok) == b.n_lines  # (ALT #1 prints a row on every line: record i is line i's)
    return int(((first["flags"] & 2) != 0).sum()), len(ok)


LIST_SAMPLES = 2500  # (closed_domains.G3_MANY_SAMPLES: the size at which the list mode has room for eight ALT indices)


def test_list_mode_lines_leave_class_lists_and_dense_lines_maps(bv, monkeypatch):
    """The regular probes' lines on the streaming chain.  At 2 500 samples a class-map slot (640 bytes) holds the class lists
    of eight ALT indices: list-mode lines whose probe stays below 9 come back with BVCF_ALLELE_CMAP_SPARSE on ALT #1.  At 260
    samples the slot (80 bytes) holds one list, and the carriers of ALT #2.. turn every line into a map whose further alleles
    are left to k_gt: no line carries the flag there.  "Some" is therefore asked of the list-mode lines of 2 500 samples.
    No line of the other densities carries the flag at either size.  (Lines of 2 600 samples are more than the ten chunks
    k_stream's pipeline takes: they are scanned one at a time, without the list mode, and have no part in this.)"""
    counts = {}
    for what, vcf in (("260 list", cd.g3_regular("list")), ("260 dense", cd.g3_regular("dense")),
                      ("2500 list", cd.g3_many(LIST_SAMPLES, "list", True)), ("2500 raw", cd.g3_many(LIST_SAMPLES, "raw", True)),
                      ("2500 dense", cd.g3_many(LIST_SAMPLES, "dense", True))):
        counts[what] = sparse_first_records(records_of(bv, monkeypatch, vcf)[0])
    print("ALT #1 records with a class list / lines:", counts)
    assert all(n == 242 for _, n in counts.values())
    assert counts["2500 list"][0] > 0
    assert counts["260 list"][0] == 0  # (one list per slot, carriers up to 9: finish_list never keeps a line as a list here)
    assert counts["260 dense"][0] == 0 and counts["2500 raw"][0] == 0 and counts["2500 dense"][0] == 0


RAW_MAX = 63  # kRawMax


def expected_raw_area(line, ns):
    """what raw_save leaves behind the class-map slot of a regular line that ended in list mode with 16..63 non-reference
    lanes: uint32 n; at +16 the lanes' map byte indices; at +16 + 4 * 64 their four field words ^ "0<sep>0<TAB>" (the
    terminator of the last field taken as its TAB, fields past the last sample as the reference)"""
    f = line.split(b"\t")[9:]
    assert len(f) == ns and all(len(x) == 3 for x in f)
    kref = bytes((0x30, f[0][1], 0x30, 0x09))
    idx, words = [], []
    for lane in range((ns + 3) // 4):
        w = []
        for s in range(4 * lane, 4 * lane + 4):
            field = f[s] + b"\t" if s < ns else kref
            w.append(int.from_bytes(bytes(x ^ y for x, y in zip(field, kref)), "little"))
        if any(w):
            idx.append(lane)
            words.append(w)
    area = np.zeros(16 + 4 * (RAW_MAX + 1) + 16 * RAW_MAX, dtype=np.uint8)
    if len(idx) > RAW_MAX:
        return area, len(idx)  # (more lanes than a raw list holds: nothing is saved)
    area[:4].view("<u4")[0] = len(idx)
    area[16:16 + 4 * len(idx)].view("<u4")[:] = idx
    at = 16 + 4 * (RAW_MAX + 1)
    area[at:at + 16 * len(idx)].view("<u4")[:] = np.array(words, dtype="<u4").reshape(-1)
    return area, len(idx)


def further_forms(bv, b, body, ns):
    """per line with records of further ALT indices that have maps of their own: "listed" when ALT #1 is a class list and the
    further alleles came from the lists behind it; for a dense map of ALT #1 "raw" when the line's entries lie behind its
    class-map slot exactly as raw_save writes them (k_gt classified them), else "no raw list": k_gt read the line again -- the
    records do not say so themselves (the offset's low bits that tell k_head are masked out of cmap_off), so this only means
    that no raw list was found: a line too dense for one, or a wave without spare slots behind the line's own.  A raw list that
    names the line's lanes but holds other words than the line's text is an error, not "no raw list"."""
    lines = body.split(b"\n")[:-1]
    forms = {"raw": 0, "no raw list": 0, "listed": 0, "none": 0}
    for i in range(b.n_lines):
        recs = b.records(i)
        further = recs[(recs["alt_idx"] > 0) & (recs["cmap_off"] != bv.NO_CMAP)]
        if len(further) == 0:
            forms["none"] += 1
        elif int(recs[0]["flags"]) & 2:
            # (finish_list: the lists of ALT #2..#8 sit behind ALT #1's; a higher index is rescanned when someone is missing)
            assert ((further["flags"][further["alt_idx"] < 8] & 2) != 0).all()
            forms["listed"] += 1
        else:
            assert ((further["flags"] & 2) == 0).all()
            want, n = expected_raw_area(lines[i], ns)
            at = int(recs[0]["cmap_off"]) + b.cmap_stride
            used = 16 + 4 * (RAW_MAX + 1) + 16 * n
            named = 16 <= n <= RAW_MAX and at + used <= len(b.cmap) and bool(
                (b.cmap[at:at + 4] == want[:4]).all() and (b.cmap[at + 16:at + 16 + 4 * n] == want[16:16 + 4 * n]).all())
            if named:
                assert (b.cmap[at + 272:at + used] == want[272:used]).all(), "line %d: a raw list with other words than the line's" % i
            forms["raw" if named else "no raw list"] += 1
    return forms


def test_further_alleles_come_from_raw_lists_and_from_rescans(bv, monkeypatch):
    """2 500 samples, the regular probes: the lines of 16..63 non-reference lanes leave their entries behind the slot for k_gt
    where the wave has slots to spare (raw_save; a list that is found is checked byte for byte against the line's text), the
    dense lines -- more than 63 lanes with a digit >= 2 -- can leave none, so their further alleles are read from the line again,
    the list-mode lines settle them from class lists (write_further_lists).  That the rows are right either way is what the
    parity runs above show; this shows that each way is taken."""
    forms = {}
    for density in cd.G3_MANY_DENSITIES:
        b, body = records_of(bv, monkeypatch, cd.g3_many(LIST_SAMPLES, density, True))
        forms[density] = further_forms(bv, b, body, LIST_SAMPLES)
    print("further alleles of the lines at 2 500 samples:", forms)
    assert forms["raw"]["raw"] > 0 and forms["dense"]["no raw list"] == 242 and forms["list"]["listed"] > 0
    assert forms["dense"]["raw"] == 0 and forms["raw"]["listed"] == 0 and forms["dense"]["listed"] == 0


# ------------------------------------------------------------------ R: REF, ALT, POS and CHROM

R_CHAINS = {"census": {"BVCF_PATH": "1"}, "streaming-head-walk": {"BVCF_PATH": "2", "BVCF_HEAD_FAST": "0"},
            "streaming-head-fast": {"BVCF_PATH": "2", "BVCF_HEAD_FAST": "1"}}
SITES_CHAINS = {"k_sites2-rendered": {"BVCF_SITES": "2", "BVCF_PACKED_SITES": "1", "BVCF_RENDER_SITES": "1"},
                "k_sites2-host-rows": {"BVCF_SITES": "2", "BVCF_PACKED_SITES": "1", "BVCF_RENDER_SITES": "0"},
                "k_sites2-unpacked": {"BVCF_SITES": "2", "BVCF_PACKED_SITES": "0", "BVCF_RENDER_SITES": "0"},
                "census": {"BVCF_SITES": "0", "BVCF_PACKED_SITES": "0", "BVCF_RENDER_SITES": "0"}}


def hold_r(bv, name):
    vcf = cd.piece(name)
    hold(bv, vcf, oracle(name))
    hold(bv, vcf, oracle(name, frozen(KEEP_ALL)), KEEP_ALL)
    hold(bv, vcf, oracle(name), max_batch_bytes=1 << 16)


@pytest.mark.parametrize("block", cd.R_BLOCKS)
@pytest.mark.parametrize("r_chain", list(R_CHAINS))
def test_ref_alt_pos_chrom_with_samples(bv, monkeypatch, r_chain, block):
    monkeypatch.setenv("BVCF_GEN_STREAM", "0")
    for k, v in R_CHAINS[r_chain].items():
        monkeypatch.setenv(k, v)
    hold_r(bv, "r-" + block)


@pytest.mark.parametrize("block", cd.R_BLOCKS)
@pytest.mark.parametrize("r_chain", ["streaming-head-walk", "streaming-head-fast"])
def test_ref_alt_pos_chrom_in_long_lines(bv, monkeypatch, r_chain, block):
    """the same with 70 samples: k_stream hands k_order the TAB bitmap of a line's head only when the head's 256-byte window
    holds no terminator, so the lines of three samples never reach k_order's fast lane; these do"""
    monkeypatch.setenv("BVCF_GEN_STREAM", "0")
    for k, v in R_CHAINS[r_chain].items():
        monkeypatch.setenv(k, v)
    hold_r(bv, "r-%s-long" % block)


@pytest.mark.parametrize("block", cd.R_BLOCKS)
@pytest.mark.parametrize("sites_chain", list(SITES_CHAINS))
def test_ref_alt_pos_chrom_sites_only(bv, monkeypatch, sites_chain, block):
    monkeypatch.delenv("BVCF_S2_CENSUS", raising=False)
    for k, v in SITES_CHAINS[sites_chain].items():
        monkeypatch.setenv(k, v)
    hold_r(bv, "r-%s-sites" % block)


def test_head_fast_lane_takes_lines_of_r(bv, monkeypatch):
    """with BVCF_HEAD_FAST=1 k_order settles plain SNP lines of R itself: fewer lines than the batch holds are left to k_head
    -- in the lines of 70 samples (those of three are shorter than the window a bitmap is made of: k_head gets them all)"""
    monkeypatch.setenv("BVCF_HEAD_FAST", "1")
    force(monkeypatch, "streaming")
    left = {}
    for ns in (cd.R_LONG_SAMPLES, cd.R_SAMPLES):
        body = b"".join(body_of(cd.r(blk, ns))[2] for blk in cd.R_BLOCKS)
        ctx = roomy_ctx(bv, 9 + ns, body, 2)
        try:
            assert ctx.path() == 2
            b = ctx.process(body)
            assert b.n_lines == body.count(b"\n")
            left[ns] = (ctx.head_left(), b.n_lines)
        finally:
            ctx.close()
    print("lines of R left to k_head / lines, by sample count:", left)
    n_snp = sum(len(ref) == 1 and len(alt) == 1 and alt in (b"A", b"C") and alt != ref
                for blk in cd.R_BLOCKS for _, pos, _, ref, alt in cd.r_records(blk))
    assert n_snp > 1365
    assert left[cd.R_LONG_SAMPLES][0] is not None and left[cd.R_LONG_SAMPLES][0] < left[cd.R_LONG_SAMPLES][1] - n_snp // 2
