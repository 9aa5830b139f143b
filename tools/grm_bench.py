#!/usr/bin/env python3
"""What does --grm cost?  (not a test): one JSON line.

  chain     a device-resident configs[2] (c3) block through the kernel chain with the GRM off and on: one block at a time
            and with the library's blocks in flight; the rows per block that carry a dense map / a short list; and the
            HIP-event time of each GRM step over one block (bvcf_bench_grm_kernels)
  e2e       the CLI on configs[2] rows from a BGZF file: plain, and the GRM-only pass --noOut --grm (the second of two runs
            each)

usage: grm_bench.py [chain|e2e|all] [ROWS]   (e2e rows, default 100 000)
BVCF_LIB / BVCF_EXE name another build of the library and the CLI (a parent commit's, for the legs without the feature): the
"on" legs and the --grm runs are then skipped."""
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
MAX_ALLELES = 524_288  # BVCF_GRM_MAX_BATCH_ROWS: what a ctx with the GRM on may reserve (the default, 2 * lines + 1024, is above it)
HAS_GRM = hasattr(bv.lib, "bvcf_enable_grm")


def chain(prof="c3"):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS, pad=bv.DEVICE_PAD)
    out = {"has_grm": HAS_GRM, "rows": ROWS}
    for tag, on in (("off", False), ("on", True)):
        if on and not HAS_GRM:
            continue
        ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, max_lines=ROWS + 64, max_alleles=MAX_ALLELES,
                     **({"grm": True} if on else {}))
        ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
        alone, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
        ctx.bench_device([t.data_ptr()], [nbytes], 6)
        flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
        out[tag] = {"alone_ms": float(np.median(alone)), "in_flight_ms": float(np.mean(flight[3:]))}
        if on:
            ctx.bench_device([t.data_ptr()], [nbytes], 1, slots=1)
            ks = [ctx.bench_grm_kernels() for _ in range(5)]
            out["kernel_ms"] = dict(zip(["k_grm_list", "k_grm_pack+k_grm_gemm", "k_grm_sparse", "k_grm_fold"],
                                        [float(x) for x in np.median(np.array(ks), axis=0)]))
            ctx.submit_device(t.data_ptr(), nbytes)
            out["dense_rows"], out["sparse_rows"] = row_forms(ctx.collect())
        ctx.close()
    if "on" in out:
        out["grm_kernels_ms_per_block"] = out["on"]["alone_ms"] - out["off"]["alone_ms"]
        out["in_flight_cost_pct"] = 100.0 * (out["on"]["in_flight_ms"] / out["off"]["in_flight_ms"] - 1.0)
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_grm_%d" % rows)
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
    if HAS_GRM:
        for _ in range(2):
            res["no_out_grm_s"] = cli(["--in", base + ".bgzf", "--noOut", "--grm", base])
        res["grm_bin_MB"] = os.path.getsize(base + ".grm.bin") / 1e6
        for sfx in (".grm.bin", ".grm.N.bin", ".grm.id"):
            os.unlink(base + sfx)
    return res


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
    out = {}
    if what in ("chain", "all"):
        out["c3"] = chain("c3")
    if what in ("e2e", "all"):
        out["e2e_c3"] = e2e(rows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
