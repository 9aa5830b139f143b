#!/usr/bin/env python3
"""What does --sampleStats cost?  (not a test): one JSON line.

  chain     device-resident configs[2] (c3) and configs[3] (c4) blocks through the kernel chain with the per-sample counts
            off and on: one block at a time (the on - off difference is the k_ss_* kernels' time per block) and with the
            library's blocks in flight; plus the rows per block that carry a dense map / a short list, and the dense-map
            bytes k_ss_dense reads
  e2e       the CLI on configs[2] rows from a BGZF file, with and without --sampleStats (the second of two runs each)

usage: sample_stats_bench.py [ROWS]   (e2e rows, default 200 000)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchgen as bg  # noqa: E402
import bgzf  # noqa: E402
import bystro_vcf_amd as bv  # noqa: E402

EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
ROWS = {"c3": 311_296, "c4": 262_144}  # bench.py's block shapes


def row_forms(b):
    """(dense rows, short-list rows) of a collected batch"""
    n = b.n_lines
    a = b.alleles
    k = np.arange(len(a))
    li = np.where(k < n, k, a["line"])
    L = b.lines[np.minimum(li, max(n - 1, 0))]
    live = (li < n) & (L["status"] == bv.LINE_OK) & (L["n_rec"] > 0) & (a["ac"] > 0) & (a["cmap_off"] != bv.NO_CMAP)
    live &= (k < n) | ((k >= L["rec_first"]) & (k - L["rec_first"] + 1 < L["n_rec"]))
    sparse = (a["flags"] & 2) != 0
    return int((live & ~sparse).sum()), int((live & sparse).sum())


def chain(prof):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS[prof], pad=bv.DEVICE_PAD)
    ns = cfg.n_samples
    stride = ((ns + 3) // 4 + 15) & ~15
    out = {}
    for tag, on in (("off", False), ("on", True)):
        ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, sample_stats=on)
        ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
        alone, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 16, slots=1)
        ctx.bench_device([t.data_ptr()], [nbytes], 6)
        flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 24)
        out[tag] = {"alone_ms": float(np.median(alone)), "in_flight_ms": float(np.mean(flight[3:]))}
        if on:
            ctx.submit_device(t.data_ptr(), nbytes)
            dense, sparse = row_forms(ctx.collect())
            out["dense_rows"], out["sparse_rows"] = dense, sparse
            out["dense_map_MB_read"] = dense * stride / 1e6
        ctx.close()
    out["k_sample_stats_us_per_block"] = 1e3 * (out["on"]["alone_ms"] - out["off"]["alone_ms"])
    out["in_flight_cost_pct"] = 100.0 * (out["on"]["in_flight_ms"] / out["off"]["in_flight_ms"] - 1.0)
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_ss_%d" % rows)
    cfg = bg.make_cfg("c3")
    if not os.path.exists(base + ".bgzf"):
        with open(base + ".bgzf", "wb") as fb:
            fb.write(bgzf.bgzf_compress(bg.header(cfg), eof_marker=False, level=1))
            for first in range(0, rows, 5_000):
                fb.write(bgzf.bgzf_compress(bg.rows_host(cfg, first, min(5_000, rows - first)), eof_marker=False, level=1))
            fb.write(bgzf.bgzf_block(b""))
    res = {"rows": rows}
    for _ in range(2):
        res["plain_s"] = cli(["--in", base + ".bgzf"])
    for _ in range(2):
        res["sample_stats_s"] = cli(["--in", base + ".bgzf", "--sampleStats", base + ".stats"])
    for _ in range(2):
        res["no_out_sample_stats_s"] = cli(["--in", base + ".bgzf", "--noOut", "--sampleStats", base + ".stats"])
    os.unlink(base + ".stats")
    return res


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    print(json.dumps({"c3": chain("c3"), "c4": chain("c4"), "e2e_c3": e2e(rows)}))


if __name__ == "__main__":
    main()
