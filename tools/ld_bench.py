#!/usr/bin/env python3
"""What do --ld / --ldPrune cost?  (not a test): one JSON line.

  chain-off     device-resident configs[2] (c3) blocks through the kernel chain without the pairs: one block at a time
                and with the library's blocks in flight
  chain-on [N]  the same with bvcf_enable_ld (window N, default 50, threshold 0.2), and the HIP-event time of the row
                index, k_bed_rows, k_ld_keys, the counting k_ld_pairs, k_ld_scan and the filling k_ld_pairs over one
                block (bvcf_bench_ld_kernels), the rows and events of the block, and the bytes of events and edge rows
                that cross to the host per block
  e2e [ROWS] [N]  the CLI on configs[2] rows from a BGZF file (default 200 000): plain and the QC-only pass
                --noOut --ld --ldPrune (the second of two runs each), with the sizes of what it wrote
  seam [N]      the host seam alone: the time of one boundary at window N (default 512) -- the pairs of a batch's first N
                rows with the N rows kept from the batch before, 2 504 samples -- which is the one serial piece

usage: ld_bench.py chain-off|chain-on|e2e|seam [...]
One leg per process: run the legs in turn, each in a fresh process.  BVCF_LIB / BVCF_EXE name another build (a parent
commit's, for chain-off and the plain e2e leg)."""
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
T6 = 200_000
HAS_LD = hasattr(bv.lib, "bvcf_enable_ld")


def chain(on, window, prof="c3"):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS, pad=bv.DEVICE_PAD)
    nh = bg.n_header_fields(cfg)
    out = {"window": window if on else 0, "samples": nh - 9, "lib": os.environ.get("BVCF_LIB", "")}
    ctx = bv.Ctx(nh, max_batch_bytes=nbytes, **({"ld": (window, T6)} if on else {}))
    if on:
        ctx.reserve_ld_events(16 << 20)
    ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
    alone, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
    ctx.bench_device([t.data_ptr()], [nbytes], 6)
    flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
    out["alone_ms"], out["in_flight_ms"] = float(np.median(alone)), float(np.mean(flight[3:]))
    out["alone_ms_all"] = [round(float(x), 4) for x in alone]
    if on:
        ctx.bench_device([t.data_ptr()], [nbytes], 1, slots=1)
        ks = [ctx.bench_ld_kernels() for _ in range(5)]
        ms = np.median(np.array([k[0] for k in ks]), axis=0)
        out["kernel_ms"] = dict(zip(["row_index", "k_bed_rows", "k_ld_keys", "k_ld_pairs_count", "k_ld_scan", "k_ld_pairs_fill"],
                                    [float(x) for x in ms]))
        out["rows"], out["events"] = ks[0][1], ks[0][2]
        ctx.submit_device(t.data_ptr(), nbytes)
        ctx.collect()
        info = ctx.ld_info()
        out["d2h_bytes"] = 32 * int(info.n_events) + 2 * int(info.n_edge) * int(info.row_bytes)
    ctx.close()
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def e2e(rows, window):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_ld_%d" % rows)
    cfg = bg.make_cfg("c3")
    if not os.path.exists(base + ".bgzf"):
        with open(base + ".bgzf", "wb") as fb:
            fb.write(bgzf.bgzf_compress(bg.header(cfg), eof_marker=False, level=1))
            for first in range(0, rows, 5_000):
                fb.write(bgzf.bgzf_compress(bg.rows_host(cfg, first, min(5_000, rows - first)), eof_marker=False, level=1))
            fb.write(bgzf.bgzf_block(b""))
    res = {"rows": rows, "window": window}
    for _ in range(2):
        res["plain_s"] = cli(["--in", base + ".bgzf"])
    if HAS_LD:
        for _ in range(2):
            res["no_out_ld_s"] = cli(["--in", base + ".bgzf", "--noOut", "--ld", base + ".ld", "--ldPrune", base, "--ldWindow", str(window)])
        for ext in (".ld", ".prune.in", ".prune.out"):
            res[ext[1:].replace(".", "_") + "_MB"] = os.path.getsize(base + ext) / 1e6
            os.unlink(base + ext)
    return res


def seam(window, ns=2504):
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 256, size=(2 * window, (ns + 3) // 4), dtype=np.uint8)
    loci = [b"chr1\t%d\tA\tG" % (100 + i) for i in range(2 * window)]
    none = np.zeros((0, 8), dtype=np.uint32)
    times = []
    for _ in range(5):
        s = bv.LdSeam(ns, window, T6)
        s.push(rows[:window], none, loci[:window])
        t0 = time.perf_counter()
        s.push(rows[window:], none, loci[window:])
        times.append(time.perf_counter() - t0)
        s.close()
    return {"window": window, "samples": ns, "pairs": window * (window + 1) // 2, "boundary_ms": 1e3 * float(np.median(times))}


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "chain-on"
    if what == "e2e":
        out = {"e2e_c3": e2e(int(sys.argv[2]) if len(sys.argv) > 2 else 200_000, int(sys.argv[3]) if len(sys.argv) > 3 else 50)}
    elif what == "seam":
        out = {"seam": seam(int(sys.argv[2]) if len(sys.argv) > 2 else 512)}
    else:
        if what == "chain-on" and not HAS_LD:
            sys.exit("this build of the library has no bvcf_enable_ld")
        out = {"c3": chain(what == "chain-on", int(sys.argv[2]) if len(sys.argv) > 2 else 50)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
