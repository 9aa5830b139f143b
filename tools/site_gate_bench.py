#!/usr/bin/env python3
"""What does the site gate (--minMaf / --maxMaf / --minMac / --maxMissing / --hwe) cost, and what does it cost when it is
off?  (not a test): one JSON line.

  resident  one device-resident block of bench.py's row model, c3 (2 504 samples, FORMAT GT: configs[2]), through the
            kernel chain, one block at a time and with three blocks in flight:
              off      this build, no gate
              cheap    this build, --minMaf 0.05 --maxMissing 0.1 --minMac 2 (k_site_gate alone)
              hwe      this build, the same and --hwe 1e-6 (k_site_gate's inline test, and k_site_hwe for the long rows)
            and, with --parent-lib (a libbvcf.so of the parent commit), the parent's chain: parent
            The hwe leg also reports the two kernels' own HIP-event times (bvcf_bench_gate_kernels).
            Every leg is a fresh child process; the legs are run in turn, --reps times over, so that a drifting box shows
            in all of them alike (medians are reported, all repetitions kept).
  e2e       the CLI as `--noOut --relatedness` over a c3 text file of --e2e-rows rows, without and with
            --minMaf 0.05 --maxMissing 0.1

usage: site_gate_bench.py [--rows N] [--e2e-rows N] [--reps R] [--parent-lib PATH] [--skip-e2e]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
CHEAP = {"minMaf": 0.05, "maxMissing": 0.1, "minMac": 2}
LEGS = {"off": (False, None), "cheap": (False, CHEAP), "hwe": (False, dict(CHEAP, hwe=1e-6)), "parent": (True, None)}


def child(leg, rows):
    """one leg in this process: the block is made on the device, the ctx created, the chain timed"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import benchgen as bg
    import bystro_vcf_amd as bv
    gate = LEGS[leg][1]
    cfg = bg.make_cfg("c3")
    t, nbytes = bg.rows_device(cfg, 0, rows, pad=bv.DEVICE_PAD)
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, n_slots=3)
    if gate:
        ctx.set_site_gate(gate)
    ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
    alone, _, counts = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
    ctx.bench_device([t.data_ptr()], [nbytes], 6)
    flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
    out = {"alone_ms": float(np.median(alone)), "in_flight_ms": float(np.mean(flight[3:])), "path": ctx.path(),
           "block_MB": nbytes / 1e6, "lines": counts[0], "records": counts[1]}
    if gate:
        ms = [ctx.bench_gate_kernels() for _ in range(5)]
        out["k_site_gate_ms"] = statistics.median(m[0] for m in ms)
        out["k_site_hwe_ms"] = statistics.median(m[1] for m in ms)
    ctx.close()
    print(json.dumps(out))


def run_leg(leg, rows, parent_lib):
    env = dict(os.environ)
    for k in ("BVCF_PATH", "BVCF_GEN_STREAM", "BVCF_WIDE"):
        env.pop(k, None)
    if LEGS[leg][0]:
        env["BVCF_LIB"] = parent_lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--rows", str(rows)], env=env,
                       capture_output=True, timeout=600)
    assert p.returncode == 0, (leg, p.stderr[-600:])
    return json.loads(p.stdout.decode().strip().split("\n")[-1])


def resident(rows, reps, parent_lib):
    legs = [k for k, v in LEGS.items() if parent_lib or not v[0]]
    runs = {k: [] for k in legs}
    for _ in range(reps):
        for k in legs:
            runs[k].append(run_leg(k, rows, parent_lib))
    out = {"rows": rows, "reps": reps, "block_MB": runs[legs[0]][0]["block_MB"], "records": runs[legs[0]][0]["records"]}
    for k in legs:
        out[k] = {"alone_ms": statistics.median(r["alone_ms"] for r in runs[k]),
                  "in_flight_ms": statistics.median(r["in_flight_ms"] for r in runs[k]),
                  "alone_ms_all": [round(r["alone_ms"], 3) for r in runs[k]],
                  "in_flight_ms_all": [round(r["in_flight_ms"], 3) for r in runs[k]], "path": runs[k][0]["path"]}
        for q in ("k_site_gate_ms", "k_site_hwe_ms"):
            if q in runs[k][0]:
                out[k][q] = statistics.median(r[q] for r in runs[k])
    for k in ("cheap", "hwe"):
        out[k + "_over_off_alone"] = out[k]["alone_ms"] / out["off"]["alone_ms"]
        out[k + "_over_off_in_flight"] = out[k]["in_flight_ms"] / out["off"]["in_flight_ms"]
    if parent_lib:
        out["off_over_parent_alone"] = out["off"]["alone_ms"] / out["parent"]["alone_ms"]
        out["off_over_parent_in_flight"] = out["off"]["in_flight_ms"] / out["parent"]["in_flight_ms"]
    return out


def e2e(rows, reps):
    sys.path.insert(0, ROOT)
    import benchgen as bg
    tmp = os.environ.get("TMPDIR", "/tmp")
    path = os.path.join(tmp, "bvcf_gate_c3_%d.vcf" % rows)
    pairs = os.path.join(tmp, "bvcf_gate_c3.pairs")
    cfg = bg.make_cfg("c3")
    if not os.path.exists(path):
        with open(path, "wb") as f:
            f.write(bg.header(cfg))
            for first in range(0, rows, 2_000):
                f.write(bg.rows_host(cfg, first, min(2_000, rows - first)))
    legs = [("plain", []), ("gated", ["--minMaf", "0.05", "--maxMissing", "0.1"])]
    runs = {k: [] for k, _ in legs}
    for _ in range(reps):
        for k, extra in legs:
            t0 = time.perf_counter()
            p = subprocess.run([EXE, "--in", path, "--noOut", "--relatedness", pairs] + extra, capture_output=True, timeout=900)
            runs[k].append(time.perf_counter() - t0)
            assert p.returncode == 0, p.stderr[-400:]
    res = {"rows": rows, "file_MB": os.path.getsize(path) / 1e6, "reps": reps}
    for k, _ in legs:
        res[k] = {"wall_s_median": statistics.median(runs[k]), "wall_s_all": [round(x, 3) for x in runs[k]]}
    os.unlink(path)
    os.unlink(pairs)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_288)  # one of bench.py's eight blocks (98 304 rows)
    ap.add_argument("--e2e-rows", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rows)
    out = {"resident": resident(a.rows, a.reps, a.parent_lib)}
    if not a.skip_e2e:
        out["e2e"] = e2e(a.e2e_rows, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
