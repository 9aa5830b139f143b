#!/usr/bin/env python3
"""What does row selection by a locus list (--keepVariants / --excludeVariants) cost, and what does it cost when it is off?
(not a test): one JSON line.

  resident  one device-resident block of bench.py's row model, c3 (2 504 samples, FORMAT GT: configs[2]), through the
            kernel chain, one block at a time and with three blocks in flight:
              off      this build, no list
              parent   with --parent-lib (a libbvcf.so of the parent commit), the parent's chain
              k3-miss .. k7-hit   this build with a keep list of 10^3, 10^6 and 10^7 entries -- `miss`: none of them a
                       locus of the block (hit rate 0); `hit`: the block's own loci first, as many as the list holds, then
                       entries that match nothing (hit rate min(1, entries / rows)).  These legs also report
                       k_variant_gate's own HIP-event time (bvcf_bench_variant_kernel), the median of five.
            Every leg is a fresh child process; the legs are run in turn, --reps times over (the list legs once: their
            number is the kernel's own), so that a drifting box shows in all of them alike (medians are reported, all
            repetitions kept).
  e2e       the CLI as `--noOut --relatedness` over a c3 text file of --e2e-rows rows, plain and with a list that keeps a
            tenth of the rows

usage: variant_list_bench.py [--rows N] [--e2e-rows N] [--reps R] [--parent-lib PATH] [--skip-e2e] [--sizes 3,6,7]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


def filler(n):
    """n entries that are no locus of any block: a chromosome the row model does not have"""
    return ("\n".join(map("chr99:{}:A:T".format, range(1, n + 1))) + "\n").encode() if n else b""


def block_loci(bv, bg, cfg, rows):
    """the locus strings of the block's rows: the second column of this build's own .bim of the same rows"""
    prefix = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_variants_block_%d" % os.getpid())
    rc, out, log, _ = bv.run_buffer(bg.header(cfg) + bg.rows_host(cfg, 0, rows), {"noOut": True, "plinkOutput": prefix})
    assert rc == 0, log
    with open(prefix + ".bim", "rb") as f:
        loci = [ln.split(b"\t")[1] for ln in f.read().split(b"\n") if ln]
    for e in (".bed", ".bim", ".fam"):
        os.unlink(prefix + e)
    return loci


def child(leg, rows):
    """one leg in this process: the block is made on the device, the ctx created, the chain timed"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import benchgen as bg
    import bystro_vcf_amd as bv
    cfg = bg.make_cfg("c3")
    out = {}
    table = None
    if leg[0] == "k":
        n = 10 ** int(leg[1])
        own = block_loci(bv, bg, cfg, rows)[:n] if leg.endswith("hit") else []
        t0 = time.perf_counter()
        table = bv.VariantTable(text=b"".join(x + b"\n" for x in own) + filler(n - len(own)))
        out.update(entries=table.n, capacity=table.capacity, table_MB=(16 * table.capacity + len(table.blob)) / 1e6,
                   build_s=time.perf_counter() - t0, own=len(set(own)))
    t, nbytes = bg.rows_device(cfg, 0, rows, pad=bv.DEVICE_PAD)
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, n_slots=3)
    if table is not None:
        ctx.set_variant_list(table)
    ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
    alone, _, counts = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
    ctx.bench_device([t.data_ptr()], [nbytes], 6)
    flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
    out.update(alone_ms=float(np.median(alone)), in_flight_ms=float(np.mean(flight[3:])), path=ctx.path(), block_MB=nbytes / 1e6,
               lines=counts[0], records=counts[1])
    if table is not None:
        ms = [ctx.bench_variant_kernel() for _ in range(6)][1:]
        out["k_variant_gate_ms"] = statistics.median(ms)
        out["k_variant_gate_ms_all"] = [round(x, 4) for x in ms]
    ctx.close()
    print(json.dumps(out))


def run_leg(leg, rows, parent_lib):
    env = dict(os.environ)
    for k in ("BVCF_PATH", "BVCF_GEN_STREAM", "BVCF_WIDE"):
        env.pop(k, None)
    if leg == "parent":
        env["BVCF_LIB"] = parent_lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--rows", str(rows)], env=env,
                       capture_output=True, timeout=900)
    assert p.returncode == 0, (leg, p.stderr[-600:])
    return json.loads(p.stdout.decode().strip().split("\n")[-1])


def resident(rows, reps, parent_lib, sizes):
    base = ["off"] + (["parent"] if parent_lib else [])
    lists = ["k%d-%s" % (s, h) for s in sizes for h in ("miss", "hit")]
    runs = {k: [] for k in base + lists}
    for rep in range(reps):
        for k in base + (lists if rep == 0 else []):
            runs[k].append(run_leg(k, rows, parent_lib))
    out = {"rows": rows, "reps": reps, "block_MB": runs["off"][0]["block_MB"], "records": runs["off"][0]["records"]}
    for k in base + lists:
        out[k] = {"alone_ms": statistics.median(r["alone_ms"] for r in runs[k]),
                  "in_flight_ms": statistics.median(r["in_flight_ms"] for r in runs[k]),
                  "alone_ms_all": [round(r["alone_ms"], 3) for r in runs[k]],
                  "in_flight_ms_all": [round(r["in_flight_ms"], 3) for r in runs[k]], "path": runs[k][0]["path"]}
        for q in ("k_variant_gate_ms", "k_variant_gate_ms_all", "entries", "capacity", "table_MB", "build_s", "own"):
            if q in runs[k][0]:
                out[k][q] = runs[k][0][q]
    if parent_lib:
        out["off_over_parent_alone"] = out["off"]["alone_ms"] / out["parent"]["alone_ms"]
        out["off_over_parent_in_flight"] = out["off"]["in_flight_ms"] / out["parent"]["in_flight_ms"]
    return out


def e2e(rows, reps):
    sys.path.insert(0, ROOT)
    import benchgen as bg
    tmp = os.environ.get("TMPDIR", "/tmp")
    path = os.path.join(tmp, "bvcf_variants_c3_%d.vcf" % rows)
    pairs, prefix, lst = (os.path.join(tmp, "bvcf_variants_c3." + x) for x in ("pairs", "plink", "list"))
    cfg = bg.make_cfg("c3")
    with open(path, "wb") as f:
        f.write(bg.header(cfg))
        for first in range(0, rows, 2_000):
            f.write(bg.rows_host(cfg, first, min(2_000, rows - first)))
    # the loci of the file's rows, as this build's own .bim has them; every tenth goes into the list
    p = subprocess.run([EXE, "--in", path, "--noOut", "--plinkOutput", prefix], capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    with open(prefix + ".bim", "rb") as f:
        loci = [ln.split(b"\t")[1] for ln in f.read().split(b"\n") if ln]
    with open(lst, "wb") as f:
        f.write(b"".join(x + b"\n" for x in loci[::10]))
    legs = [("plain", []), ("tenth", ["--keepVariants", lst])]
    runs = {k: [] for k, _ in legs}
    for _ in range(reps):
        for k, extra in legs:
            t0 = time.perf_counter()
            p = subprocess.run([EXE, "--in", path, "--noOut", "--relatedness", pairs] + extra, capture_output=True, timeout=900)
            runs[k].append(time.perf_counter() - t0)
            assert p.returncode == 0, p.stderr[-400:]
    res = {"rows": rows, "file_MB": os.path.getsize(path) / 1e6, "reps": reps, "file_rows": len(loci), "listed": len(set(loci[::10]))}
    for k, _ in legs:
        res[k] = {"wall_s_median": statistics.median(runs[k]), "wall_s_all": [round(x, 3) for x in runs[k]]}
    for x in [path, pairs, lst] + [prefix + e for e in (".bed", ".bim", ".fam")]:
        os.unlink(x)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_288)  # one of bench.py's eight blocks (98 304 rows)
    ap.add_argument("--e2e-rows", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--sizes", default="3,6,7")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rows)
    out = {"resident": resident(a.rows, a.reps, a.parent_lib, [int(s) for s in a.sizes.split(",") if s])}
    if not a.skip_e2e:
        out["e2e"] = e2e(a.e2e_rows, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
