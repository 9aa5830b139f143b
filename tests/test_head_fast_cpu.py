"""k_order's fast lane, run on the host (bvcf_head_fast_line, include/bvcf_plan.h), against the oracle's rows and log.

The lane settles a plain SNP line -- one-byte REF, one-byte ACGT ALT that differs, a FILTER value it can decide, every
bounding TAB in the line's first 64 bytes -- from the entry, the TAB bitmap and the head k_stream leaves; k_head takes the
rest.  For every crafted line of headfast_cases, at every ls & 3: the lane declines, or what it computed is what the
oracle prints for the line.  It must never disagree; the lines marked so must be settled, so that the check is not empty."""
import numpy as np
import pytest

import headfast_cases as hc
import oracle_lib as orc


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


CASES = hc.cases()


def run_lane(bv, ln, sh, allow, exclude, g=7):
    """the line at block offset ls with ls & 3 == sh, in front of it the end of another line -> (verdict, L, A, ls, text)"""
    ls = 4096 + sh
    text = b"x" * (ls - 1) + b"\n" + ln + b"\n" + hc.line() + b"\n"
    bits = hc.tab_bits(text, ls)
    len_flags = len(ln) | (bv.HAS_HEAD_BITS if bits else 0)
    v, L, A = bv.head_fast_line(text[ls:ls + 80], ls, len_flags, hc.counts(), 0x1230 | 1, bits or [0] * 8, g, hc.N_HEADER, allow, exclude)
    return v, L, A, ls, text


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_lane_declines_or_agrees_with_the_oracle(bv, case):
    name, ln, allow, exclude, expect = case
    rc, rows, log, n = orc.run(hc.header() + ln + b"\n", {"allow": allow, "exclude": exclude})
    assert rc == 0 and n == 1
    rows = rows.split(b"\n")[:-1]
    f = ln.split(b"\t")
    for sh in range(4):
        v, L, A, ls, text = run_lane(bv, ln, sh, allow, exclude)
        if expect is not None:
            assert v == {"pass": bv.HEAD_FAST_PASS, "filter": bv.HEAD_FAST_FILTER, "decline": bv.HEAD_FAST_DECLINE}[expect], (name, sh, v)
        if v == bv.HEAD_FAST_DECLINE:
            continue
        # ---- the line record: where the fields are
        assert int(L["off"]) == ls and int(L["len"]) == len(ln)
        ends = np.cumsum([len(x) + 1 for x in f[:9]]) - 1
        assert L["fend"].tolist() == ends.tolist()
        assert int(L["gt_task"]) == 7 and int(L["rec_first"]) == 0 and int(L["site_type"]) == 0
        if v == bv.HEAD_FAST_FILTER:
            # dropped by the FILTER gate (main.go:447-454): no row, no message
            assert rows == [] and log == "", (name, rows, log)
            assert int(L["status"]) == bv.LINE_FILTER and int(L["n_rec"]) == 0 and int(L["n_fields"]) == 0
            continue
        assert int(L["status"]) == bv.LINE_OK and int(L["n_rec"]) == 1 and int(L["n_fields"]) == hc.N_HEADER
        # ---- the record against the oracle's row: chrom, pos, type, ref, alt, trTv ... ac, an
        assert log == "" and len(rows) == 1, (name, rows, log)
        want = rows[0].split(b"\t")
        chrom = f[0] if f[0].startswith(b"chr") else b"chr" + f[0]
        assert int(A["flags"]) & 1, "the position is the POS field verbatim"
        got = [chrom, f[1], b"SNP", bytes([int(A["ref"])]), bytes([int(A["alt_base"])]), b"%d" % int(A["trtv"])]
        assert want[:6] == got, (name, want[:6], got)
        ac, an, het, hom, miss = hc.counts()
        assert [int(A[k]) for k in ("ac", "an", "n_het", "n_hom", "n_miss")] == [ac, an, het, hom, miss]
        assert want[12:14] == [b"%d" % ac, b"%d" % an]
        assert (int(A["line"]), int(A["alt_idx"]), int(A["alt_off"]), int(A["alt_len"]), int(A["kind"]), int(A["site_type"]),
                int(A["gt_task"]), int(A["pos"])) == (7, 0, 0, 1, 0, 0, 7, 0)
        # the class-map offset without its encoding bits; bit 0 said "a class list"
        assert int(A["cmap_off"]) == 0x1230 and int(A["flags"]) == 3


def test_every_entry_flag_declines(bv):
    ln = hc.line()
    ls = 4096
    text = b"x" * (ls - 1) + b"\n" + ln + b"\n" + ln + b"\n"
    bits = hc.tab_bits(text, ls)
    ok = len(ln) | bv.HAS_HEAD_BITS
    c = hc.counts()
    assert bv.head_fast_line(text[ls:ls + 80], ls, ok, c, bv.NO_CMAP, bits, 0, hc.N_HEADER)[0] == bv.HEAD_FAST_PASS
    assert bv.head_fast_line(text[ls:ls + 80], ls, len(ln), c, bv.NO_CMAP, bits, 0, hc.N_HEADER)[0] == bv.HEAD_FAST_DECLINE
    assert bv.head_fast_line(text[ls:ls + 80], ls, ok | bv.NOT_REGULAR, c, bv.NO_CMAP, bits, 0, hc.N_HEADER)[0] == bv.HEAD_FAST_DECLINE
    assert bv.head_fast_line(text[ls:ls + 80], ls, ok, c[:4] + [bv.DEFERRED], bv.NO_CMAP, bits, 0, hc.N_HEADER)[0] == bv.HEAD_FAST_DECLINE
    assert bv.head_fast_line(text[ls:ls + 80], ls, ok, c, bv.NO_CMAP, bits, 0, 9)[0] == bv.HEAD_FAST_DECLINE
    # fewer than nine TABs in the bitmap
    few = [bits[0] & 0xFFFF] + [0] * 7
    assert 0 < bin(few[0]).count("1") < 9
    assert bv.head_fast_line(text[ls:ls + 80], ls, ok, c, bv.NO_CMAP, few, 0, hc.N_HEADER)[0] == bv.HEAD_FAST_DECLINE
    # no class map: the record says so, and is not a class list
    v, L, A = bv.head_fast_line(text[ls:ls + 80], ls, ok, c, bv.NO_CMAP, bits, 0, hc.N_HEADER)
    assert int(A["cmap_off"]) == bv.NO_CMAP and int(A["flags"]) == 1
    # a dense map (bit 0 clear, other encoding bits set)
    v, L, A = bv.head_fast_line(text[ls:ls + 80], ls, ok, c, 0x40 | 2, bits, 0, hc.N_HEADER)
    assert int(A["cmap_off"]) == 0x40 and int(A["flags"]) == 1
