#!/usr/bin/env python3
"""What does --relatedness cost?  (not a test): one JSON line.

  chain     device-resident configs[2] (c3) blocks through the kernel chain with the pair counts off and on: one block at a
            time and with the library's blocks in flight; the rows per block that carry a dense map / a short list; and the
            HIP-event time of each pair kernel over one block (bvcf_bench_pair_kernels)
  e2e       the CLI on configs[2] rows from a BGZF file: plain, and the QC-only pass --noOut --relatedness (the second of
            two runs each)

usage: pair_stats_bench.py [chain|e2e|all] [ROWS]   (e2e rows, default 200 000)
BVCF_LIB names another build of the library (a parent commit's, for the legs without the feature): the "on" legs and the
--relatedness runs are then skipped."""
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
from sample_stats_bench import row_forms  # noqa: E402

EXE = os.environ.get("BVCF_EXE") or os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
ROWS = 311_296  # bench.py's configs[2] block
HAS_PAIRS = hasattr(bv.lib, "bvcf_enable_pair_stats")


def chain(prof="c3"):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS, pad=bv.DEVICE_PAD)
    out = {"has_pairs": HAS_PAIRS}
    for tag, on in (("off", False), ("on", True)):
        if on and not HAS_PAIRS:
            continue
        ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, **({"pair_stats": True} if on else {}))
        ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
        alone, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
        ctx.bench_device([t.data_ptr()], [nbytes], 6)
        flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
        out[tag] = {"alone_ms": float(np.median(alone)), "in_flight_ms": float(np.mean(flight[3:]))}
        if on:
            ctx.bench_device([t.data_ptr()], [nbytes], 1, slots=1)
            ks = [ctx.bench_pair_kernels() for _ in range(5)]
            out["kernel_ms"] = dict(zip(["k_pr_planes", "k_pr_gemm", "k_pr_sparse", "k_pr_fold"],
                                        [float(x) for x in np.median(np.array(ks), axis=0)]))
            ctx.submit_device(t.data_ptr(), nbytes)
            out["dense_rows"], out["sparse_rows"] = row_forms(ctx.collect())
        ctx.close()
    if "on" in out:
        out["pair_kernels_ms_per_block"] = out["on"]["alone_ms"] - out["off"]["alone_ms"]
        out["in_flight_cost_pct"] = 100.0 * (out["on"]["in_flight_ms"] / out["off"]["in_flight_ms"] - 1.0)
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_pr_%d" % rows)
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
    if HAS_PAIRS:
        for _ in range(2):
            res["no_out_relatedness_s"] = cli(["--in", base + ".bgzf", "--noOut", "--relatedness", base + ".pairs"])
        res["pairs_file_MB"] = os.path.getsize(base + ".pairs") / 1e6
        os.unlink(base + ".pairs")
    return res


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    out = {}
    if what in ("chain", "all"):
        out["c3"] = chain("c3")
    if what in ("e2e", "all"):
        out["e2e_c3"] = e2e(rows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
