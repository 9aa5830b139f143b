"""The whole-block comparator of tests/blockcheck.py (host only): a one-byte change deep inside a bench-size output is
reported with its block, row, byte offset and field."""
import numpy as np
import pytest

import blockcheck as bc


def test_one_changed_byte_in_row_300000_is_reported():
    import benchgen as bg
    cfg = bg.make_cfg("c2")
    vcf = bg.header(cfg) + bg.rows_host(cfg, 0, 400_000)
    rc, want, log, n = bc.run_oracle(np.frombuffer(vcf, np.uint8))
    assert rc == 0 and n == 400_000
    bc.compare(want, log, bytes(want), log, "block 0")  # equal: no report
    start = 0
    for _ in range(300_000):
        start = want.index(b"\n", start) + 1
    fields = want[start:want.index(b"\n", start)].split(b"\t")
    off = start + sum(len(f) + 1 for f in fields[:4])  # the first byte of the alt field
    got = bytearray(want)
    got[off] ^= 0x01
    with pytest.raises(AssertionError) as e:
        bc.compare(want, log, bytes(got), log, "block 7")
    msg = str(e.value)
    assert msg.startswith("block 7: TSV row 300000 differs at byte %d " % off), msg
    assert "field 4 alt" in msg and repr(fields[4])[2:-1] in msg, msg
    # a missing tail and a log line
    with pytest.raises(AssertionError, match="block 1: TSV row 399999 differs"):
        bc.compare(want, log, want[:-3], log, "block 1")
    with pytest.raises(AssertionError, match="block 2: log line 0 differs"):
        bc.compare(want, log, want, log + "x\n", "block 2")


def test_expected_sample_counts_of_dense_and_short_maps():
    """the numpy table of a hand-made batch: a dense map, a short list, a row with ac == 0 and a failed line"""
    import bystro_vcf_amd as bv

    class B:
        pass
    ns = 7
    b = B()
    b.n_samples, b.n_lines = ns, 4
    b.lines = np.zeros(4, dtype=bv.LINE_DTYPE)
    b.lines["n_rec"] = [1, 2, 1, 1]
    b.lines["rec_first"] = [0, 4, 0, 0]
    b.lines["status"] = [bv.LINE_OK, bv.LINE_OK, bv.LINE_OK, bv.LINE_FIELDS]
    b.alleles = np.zeros(5, dtype=bv.ALLELE_DTYPE)
    b.alleles["ac"] = [3, 1, 0, 2, 1]
    b.alleles["line"] = [0, 1, 2, 3, 1]
    b.alleles["trtv"] = [1, 2, 1, 1, 0]
    b.alleles["cmap_off"] = [0, 64, 0, 0, 128]
    b.alleles["flags"] = [0, 2, 0, 0, 0]
    cmap = np.zeros(192, dtype=np.uint8)
    dense = [1, 2, 0, 3, 0, 0, 1]  # classes of samples 0..6
    for s, c in enumerate(dense):
        cmap[s // 4] |= c << (2 * (s % 4))
    cmap[64:76].view("<u4")[:] = [2, (1 << 8) | (1 << 2), (0 << 8) | 3]  # sample 5 het, sample 0 missing
    cmap[128 + 1] = 2 << 4  # slot 4, dense: sample 6 hom
    b.cmap = cmap
    got = bc.expected_sample_counts(b)
    want = np.zeros((ns, 6), dtype=np.uint64)
    want[:, 5] = 3
    for s, c in enumerate(dense):
        if c:
            want[s, c - 1] += 1
            if c < 3:
                want[s, 3] += 1
    want[5, 0] += 1
    want[5, 4] += 1
    want[0, 2] += 1
    want[6, 1] += 1
    assert got.tolist() == want.tolist()
