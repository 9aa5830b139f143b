#!/usr/bin/env python3
"""What does row selection by genomic interval (--regions / --excludeRegions) cost, and what does it cost when it is off?
(not a test): one JSON line.

  resident  one device-resident block of bench.py's row model, c3 (2 504 samples, FORMAT GT: configs[2]), through the
            kernel chain, one block at a time and with three blocks in flight:
              off      this build, no regions
              parent   with --parent-lib (a libbvcf.so of the parent commit), the parent's chain
              i1 / i3 / i6   this build with a keep set of 1, 10^3 and 10^6 intervals on the block's chromosome: one
                       interval over the middle half of the block's span; 10^3 spread evenly over it, each half a step
                       wide; 10^6 likewise (every four bases at least: a short block's span is then outrun)
              c25      10^3 such intervals on each of 25 chromosomes, as a BED
              *-kx     the same keep set beside an exclude set of the same intervals moved on by a quarter of a step
            The region legs also report k_region_gate's own HIP-event time (bvcf_bench_region_kernel), the median of
            five, and how many rows the set kept.
            Every leg is a fresh child process; the legs are run in turn, --reps times over (the region legs once: their
            number is the kernel's own), so that a drifting box shows in all of them alike (medians are reported, all
            repetitions kept).

usage: region_bench.py [--rows N (311296: one of bench.py's blocks)] [--reps R] [--parent-lib PATH] [--legs i1,i3,i6,c25,i3-kx,i6-kx,c25-kx]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHROMS = [str(c) for c in range(1, 23)] + ["X", "Y", "M"]


def block_span(bv, bg, cfg, rows):
    """(chrom, lo, hi) of the block's rows, whose positions ascend: from the second column of this build's own .bim of the
    block's first and last 64 lines"""
    prefix = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_regions_block_%d" % os.getpid())
    n = min(64, rows)
    rc, out, log, _ = bv.run_buffer(bg.header(cfg) + bg.rows_host(cfg, 0, n) + bg.rows_host(cfg, rows - n, n), {"noOut": True, "plinkOutput": prefix})
    assert rc == 0, log
    with open(prefix + ".bim", "rb") as f:
        loci = [ln.split(b"\t")[1].split(b":") for ln in f.read().split(b"\n") if ln]
    for e in (".bed", ".bim", ".fam"):
        os.unlink(prefix + e)
    pos = [int(x[1]) for x in loci]
    return loci[0][0], min(pos), max(pos)


def bed_of(chroms, lo, n, step, width, shift=0):
    """n intervals of `width` bases every `step` from lo + shift on, on every chromosome of chroms (BED: 0-based half-open)"""
    return b"".join(b"%s\t%d\t%d\n" % (c, lo + shift + j * step - 1, lo + shift + j * step - 1 + width) for c in chroms for j in range(n))


def sets_of(leg, chrom, lo, hi):
    """-> (keep BED, exclude BED or None)"""
    kind, kx = (leg[:-3], True) if leg.endswith("-kx") else (leg, False)
    span = hi - lo + 1
    if kind == "i1":
        n, step, width, chroms = 1, span, span // 2, [chrom]
        keep = bed_of(chroms, lo + span // 4, n, step, width)
    elif kind == "i6":
        n, step, chroms = 10 ** 6, max(span // 10 ** 6, 4), [chrom]
        width = step // 2
        keep = bed_of(chroms, lo, n, step, width)
    else:
        n, step, chroms = 1000, max(span // 1000, 2), [chrom] if kind == "i3" else [chrom] + [c.encode() for c in CHROMS if c.encode() != chrom[3:]]
        width = step // 2
        keep = bed_of(chroms, lo, n, step, width)
    excl = bed_of(chroms, lo + (span // 4 if kind == "i1" else 0), n, step, max(width // 2, 1), shift=max(step // 4, 1)) if kx else None
    return keep, excl


def child(leg, rows):
    """one leg in this process: the block is made on the device, the ctx created, the chain timed"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import benchgen as bg
    import bystro_vcf_amd as bv
    cfg = bg.make_cfg("c3")
    out = {}
    table = None
    if leg not in ("off", "parent"):
        chrom, lo, hi = block_span(bv, bg, cfg, rows)
        keep, excl = sets_of(leg, chrom, lo, hi)
        t0 = time.perf_counter()
        table = bv.RegionTable(keep_bed=keep, exclude_bed=excl)
        out.update(keep_intervals=table.n_keep, exclude_intervals=table.n_exclude, chroms=table.n_chroms,
                   table_MB=(32 * table.capacity + len(table.blob) + 16 * (table.n_keep + table.n_exclude)) / 1e6,
                   build_s=time.perf_counter() - t0, span=[lo, hi])
    t, nbytes = bg.rows_device(cfg, 0, rows, pad=bv.DEVICE_PAD)
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, n_slots=3)
    if table is not None:
        ctx.set_region_table(table)
    ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
    alone, _, counts = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
    ctx.bench_device([t.data_ptr()], [nbytes], 6)
    flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
    out.update(alone_ms=float(np.median(alone)), in_flight_ms=float(np.mean(flight[3:])), path=ctx.path(), block_MB=nbytes / 1e6,
               lines=counts[0], records=counts[1])
    if table is not None:
        ms = [ctx.bench_region_kernel() for _ in range(6)][1:]
        out["k_region_gate_ms"] = statistics.median(ms)
        out["k_region_gate_ms_all"] = [round(x, 4) for x in ms]
    ctx.close()
    if table is not None:  # (sixteen samples of 64 lines across the block on the product path, on a ctx of its own: what the set keeps)
        ctx = bv.Ctx(bg.n_header_fields(cfg), regions=table)
        kept = [0, 0]
        for first in range(0, max(rows - 64, 1), max(rows // 16, 1)):
            c = ctx.process(bg.rows_host(cfg, first, min(64, rows))).region_counts
            kept = [kept[0] + c[1], kept[1] + c[0]]
        out["kept_of_examined"] = kept
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


def resident(rows, reps, parent_lib, legs):
    base = ["off"] + (["parent"] if parent_lib else [])
    runs = {k: [] for k in base + legs}
    for rep in range(reps):
        for k in base + (legs if rep == 0 else []):
            runs[k].append(run_leg(k, rows, parent_lib))
    out = {"rows": rows, "reps": reps, "block_MB": runs["off"][0]["block_MB"], "records": runs["off"][0]["records"]}
    for k in base + legs:
        out[k] = {"alone_ms": statistics.median(r["alone_ms"] for r in runs[k]),
                  "in_flight_ms": statistics.median(r["in_flight_ms"] for r in runs[k]),
                  "alone_ms_all": [round(r["alone_ms"], 3) for r in runs[k]],
                  "in_flight_ms_all": [round(r["in_flight_ms"], 3) for r in runs[k]], "path": runs[k][0]["path"]}
        for q in ("k_region_gate_ms", "k_region_gate_ms_all", "keep_intervals", "exclude_intervals", "chroms", "table_MB", "build_s",
                  "kept_of_examined", "span"):
            if q in runs[k][0]:
                out[k][q] = runs[k][0][q]
    if parent_lib:
        out["off_over_parent_alone"] = out["off"]["alone_ms"] / out["parent"]["alone_ms"]
        out["off_over_parent_in_flight"] = out["off"]["in_flight_ms"] / out["parent"]["in_flight_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_288)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--legs", default="i1,i3,i6,c25,i1-kx,i3-kx,i6-kx,c25-kx")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rows)
    print(json.dumps({"resident": resident(a.rows, a.reps, a.parent_lib, [s for s in a.legs.split(",") if s])}))


if __name__ == "__main__":
    main()
