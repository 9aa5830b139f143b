"""Whole-batch checks of device-resident blocks against the CPU oracle.  Test infrastructure only.

A block (bench.py's shapes: up to 3.2 GB) is copied to the host once, behind its header, into one buffer that both the
oracle and bvcf_format_tsv read; the oracle's output for a block is kept as a digest only, so that several device paths
over the same block pay for one oracle run and one block's text is on the host at a time.  expected_sample_counts is the
--sampleStats table of a collected Batch in numpy, from the class maps alone (no k_ss_* kernel involved)."""
import ctypes as C
import hashlib

import numpy as np

import oracle_lib as orc

THREADS = 16  # the oracle's and the formatter's threads (a GPU box gives a command 16 CPUs)
SHOW = 300    # bytes of a row shown in a mismatch report


def host_copy(t, nbytes, header):
    """(buffer, n_header): the header, then the device tensor's first nbytes -- one device-to-host copy into the buffer"""
    import torch
    buf = torch.empty(len(header) + nbytes, dtype=torch.uint8)
    buf[:len(header)] = torch.frombuffer(bytearray(header), dtype=torch.uint8)
    buf[len(header):].copy_(t[:nbytes])
    return buf.numpy(), len(header)


def block_view(buf, n_header):
    """the block's bytes inside a host_copy buffer (no copy)"""
    return memoryview(buf)[n_header:]


def run_oracle(buf, cfg=None):
    """orc.run on a numpy buffer without copying it -> (rc, TSV body, log text, rows)"""
    c = orc.make_config(cfg, THREADS)
    out, err = C.c_void_p(), C.c_void_p()
    n_out, n_err, n_rows = C.c_size_t(), C.c_size_t(), C.c_uint64()
    L = orc.lib()
    rc = L.orc_run(C.byref(c), C.cast(buf.ctypes.data, C.c_char_p), len(buf), C.byref(out), C.byref(n_out), C.byref(err),
                   C.byref(n_err), C.byref(n_rows))
    try:
        o = C.string_at(out, n_out.value)
        e = C.string_at(err, n_err.value).decode(errors="replace")
    finally:
        L.orc_free(out)
        L.orc_free(err)
    return rc, o, e, n_rows.value


def digest(b):
    return hashlib.sha1(b).hexdigest()


class Oracle:
    """the oracle's (TSV digest, length, log, rows) per block key, computed on first use"""

    def __init__(self):
        self.seen = {}

    def expect(self, key, buf, cfg=None):
        if key not in self.seen:
            rc, out, log, n = run_oracle(buf, cfg)
            assert rc == 0, log[-500:]
            self.seen[key] = (digest(out), len(out), log, n)
        return self.seen[key]

    def check(self, key, buf, cfg, got_tsv, got_log, what):
        """the formatted batch equals the oracle's output for the block, byte for byte"""
        d, n, log, _ = self.expect(key, buf, cfg)
        if len(got_tsv) == n and digest(got_tsv) == d and got_log == log:
            return
        rc, out, log, _ = run_oracle(buf, cfg)  # (a mismatch: the bytes themselves, for the report)
        compare(out, log, got_tsv, got_log, what, cfg)
        raise AssertionError("%s: the oracle's output changed between runs" % what)


def first_difference(a, b):
    """the first byte offset at which a and b differ (None when they are equal)"""
    if a == b:
        return None
    m = min(len(a), len(b))
    x, y = np.frombuffer(a, np.uint8, m), np.frombuffer(b, np.uint8, m)
    step = 1 << 24
    for lo in range(0, m, step):
        d = np.flatnonzero(x[lo:lo + step] != y[lo:lo + step])
        if len(d):
            return lo + int(d[0])
    return m


def compare(want_tsv, want_log, got_tsv, got_log, what, cfg=None):
    """assert the device's TSV and log equal the oracle's; a mismatch names the block, the row (line index of the
    output), the byte offset, the field and both rows (truncated)"""
    import bystro_vcf_amd as bv
    off = first_difference(want_tsv, got_tsv)
    if off is not None:
        start = want_tsv.rfind(b"\n", 0, off) + 1
        row = want_tsv.count(b"\n", 0, start)
        col = want_tsv.count(b"\t", start, off)
        names = bv.string_header(cfg).split("\t")
        field = names[col] if col < len(names) else "#%d" % col

        def line(b):
            e = b.find(b"\n", start)
            return b[start:e if e >= 0 else len(b)][:SHOW]
        raise AssertionError("%s: TSV row %d differs at byte %d (row byte %d, field %d %s; %d vs %d bytes in all):\n"
                             "oracle: %r\nhip:    %r" % (what, row, off, off - start, col, field, len(want_tsv), len(got_tsv),
                                                         line(want_tsv), line(got_tsv)))
    if got_log != want_log:
        a, b = want_log.split("\n"), got_log.split("\n")
        i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError("%s: log line %d differs (%d vs %d lines):\noracle: %r\nhip:    %r"
                             % (what, i, len(a), len(b), (a[i] if i < len(a) else None), (b[i] if i < len(b) else None)))


def sample_names(header):
    """the normalised sample names of a header (parse.NormalizeHeader: '.' -> '_')"""
    for ln in header.split(b"\n"):
        if ln.startswith(b"#CHROM"):
            return [x.replace(b".", b"_") for x in ln.rstrip(b"\r").split(b"\t")[9:]]
    return []


def row_records(b):
    """(slots, dense) over b.alleles: the slots that are TSV rows under include/bvcf.h's rule for the per-sample table
    (an output record of a line with status OK, ac > 0), and which of them carry a dense map"""
    import bystro_vcf_amd as bv
    n = int(b.n_lines)
    a = b.alleles
    k = np.arange(len(a))
    li = np.where(k < n, k, a["line"])
    L = b.lines[np.minimum(li, max(n - 1, 0))]
    row = (li < n) & (L["status"] == bv.LINE_OK) & (L["n_rec"] > 0) & (a["ac"] > 0)
    row &= (k < n) | ((k >= L["rec_first"]) & (k - L["rec_first"] + 1 < L["n_rec"]))
    slots = np.flatnonzero(row)
    mapped = a["cmap_off"][slots] != bv.NO_CMAP
    return slots, mapped


def expected_sample_counts(b, chunk=8192):
    """uint64 (n_samples, 6) -- het, hom, missing, transitions, transversions, rows -- of one collected Batch, counted
    with numpy from its class maps: dense maps by a 2-D gather, short lists from their entries"""
    ns = int(b.n_samples)
    out = np.zeros((ns, 6), dtype=np.uint64)
    slots, mapped = row_records(b)
    out[:, 5] = len(slots)
    if not ns:
        return out
    a = b.alleles[slots[mapped]]
    sparse = (a["flags"] & 2) != 0
    nbytes = (ns + 3) // 4
    shifts = np.array([0, 2, 4, 6], dtype=np.uint8)

    def add(cls, trtv_of_rows):
        # cls: (rows, ns) class codes
        for q in (1, 2, 3):
            out[:, q - 1] += (cls == q).sum(axis=0, dtype=np.uint64)
        called = (cls == 1) | (cls == 2)
        for t, col in ((1, 3), (2, 4)):
            out[:, col] += called[trtv_of_rows == t].sum(axis=0, dtype=np.uint64)

    dense = a[~sparse]
    for lo in range(0, len(dense), chunk):
        d = dense[lo:lo + chunk]
        m = b.cmap[d["cmap_off"].astype(np.int64)[:, None] + np.arange(nbytes)]
        cls = ((m[:, :, None] >> shifts) & 3).reshape(len(d), -1)[:, :ns]
        add(cls, d["trtv"])
    sp = a[sparse]
    if len(sp):
        words = b.cmap[sp["cmap_off"].astype(np.int64)[:, None] + np.arange(64)].copy().view("<u4")
        cnt = words[:, 0]
        e = words[:, 1:]
        valid = np.arange(e.shape[1])[None, :] < cnt[:, None]
        rows = np.broadcast_to(np.arange(len(sp))[:, None], e.shape)[valid]
        e = e[valid]
        byte_i, byte = (e >> 8).astype(np.int64), (e & 0xFF).astype(np.uint8)
        for j in range(4):
            s = 4 * byte_i + j
            c = (byte >> (2 * j)) & 3
            keep = s < ns
            for q in (1, 2, 3):
                sel = keep & (c == q)
                out[:, q - 1] += np.bincount(s[sel], minlength=ns).astype(np.uint64)
            for t, col in ((1, 3), (2, 4)):
                sel = keep & ((c == 1) | (c == 2)) & (sp["trtv"][rows] == t)
                out[:, col] += np.bincount(s[sel], minlength=ns).astype(np.uint64)
    return out
