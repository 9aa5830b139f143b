#!/usr/bin/env python3
"""What does --plinkOutput cost?  (not a test): one JSON line.

  chain-off   device-resident configs[2] (c3) blocks through the kernel chain without the .bed rows: one block at a time
              and with the library's blocks in flight
  chain-on    the same with bvcf_enable_bed_rows, and the HIP-event time of the row index (k_bed_count + k_bed_scan + k_bed_index) and of
              k_bed_rows over one block (bvcf_bench_bed_kernels), the rows and bytes it wrote, the bytes per second that
              makes, and the bytes of rows that cross to the host per block
  e2e [ROWS]  the CLI on configs[2] rows from a BGZF file (default 200 000): plain, --noOut --dosageOutput and the
              conversion-only pass --noOut --plinkOutput (the second of two runs each), with the sizes of what they wrote

usage: bed_rows_bench.py chain-off|chain-on|e2e [ROWS]
One leg per process: run the legs in turn, each in a fresh process.  BVCF_LIB / BVCF_EXE name another build (a parent
commit's, for chain-off and the e2e legs without the feature)."""
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

EXE = os.environ.get("BVCF_EXE") or os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
ROWS = 311_296  # bench.py's configs[2] block
HAS_BED = hasattr(bv.lib, "bvcf_enable_bed_rows")


def chain(on, prof="c3"):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS, pad=bv.DEVICE_PAD)
    out = {"bed_rows": on, "lib": os.environ.get("BVCF_LIB", "")}
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, **({"bed_rows": True} if on else {}))
    ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
    alone, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
    ctx.bench_device([t.data_ptr()], [nbytes], 6)
    flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
    out["alone_ms"], out["in_flight_ms"] = float(np.median(alone)), float(np.mean(flight[3:]))
    if on:
        ctx.bench_device([t.data_ptr()], [nbytes], 1, slots=1)
        ks = [ctx.bench_bed_kernels() for _ in range(7)]
        ms = np.median(np.array([k[0] for k in ks]), axis=0)
        out["kernel_ms"] = {"row_index": float(ms[0]), "k_bed_rows": float(ms[1])}
        out["rows"], out["bed_bytes"] = ks[0][1], ks[0][2]
        out["k_bed_rows_write_GBps"] = ks[0][2] / (float(ms[1]) * 1e-3) / 1e9 if ms[1] > 0 else None
        # what crosses to the host per block: the rows instead of the class maps
        ctx.submit_device(t.data_ptr(), nbytes)
        ctx.collect()
        out["d2h_bed_bytes"] = int(ctx.bed_rows_info().need_bytes)
    ctx.close()
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_bed_%d" % rows)
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
        res["no_out_dosage_s"] = cli(["--in", base + ".bgzf", "--noOut", "--dosageOutput", base + ".arrow"])
    res["dosage_file_MB"] = os.path.getsize(base + ".arrow") / 1e6
    os.unlink(base + ".arrow")
    if HAS_BED:
        for _ in range(2):
            res["no_out_plink_s"] = cli(["--in", base + ".bgzf", "--noOut", "--plinkOutput", base])
        res["bed_file_MB"] = os.path.getsize(base + ".bed") / 1e6
        res["bim_file_MB"] = os.path.getsize(base + ".bim") / 1e6
        for ext in (".bed", ".bim", ".fam"):
            os.unlink(base + ext)
    return res


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "chain-on"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    if what == "e2e":
        out = {"e2e_c3": e2e(rows)}
    else:
        if what == "chain-on" and not HAS_BED:
            sys.exit("this build of the library has no bvcf_enable_bed_rows")
        out = {"c3": chain(what == "chain-on")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
