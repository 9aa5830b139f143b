#!/usr/bin/env python3
"""What does --minGQ / --minDP cost?  (not a test): one JSON line.

  resident  one device-resident GT:DP:GQ block of bench.py's c5 row model through the kernel chain, one block at a time
            and with the library's blocks in flight:
              filtered       this build, min_gq = 20 (the census chain with k_gt_filter)
              census_off     this build, thresholds off, BVCF_PATH=1 (the census chain with k_gt's general scan)
              default_off    this build, thresholds off, the streaming-general chain the CLI picks for such a file
            and, with --parent-lib (a libbvcf.so of the parent commit), the same two thresholds-off chains of the parent:
              parent_census, parent_default
            Every leg is a fresh child process; the legs are run in turn, --reps times over, so that a drifting box shows
            in all of them alike (medians are reported, all repetitions kept).
  e2e       the CLI over a c5 text file with and without --minGQ 20 (BVCF_TIMING=json: the stage split of each run), and
            the parent's CLI (--parent-exe) over the same file

usage: gt_filter_bench.py [--rows N] [--e2e-rows N] [--reps R] [--parent-lib PATH] [--parent-exe PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")

LEGS = {  # name -> (parent build?, Ctx keywords, environment)
    "filtered": (False, {"min_gq": 20}, {}),
    "census_off": (False, {}, {"BVCF_PATH": "1"}),
    "default_off": (False, {"path": 3}, {}),
    "parent_census": (True, {}, {"BVCF_PATH": "1"}),
    "parent_default": (True, {"path": 3}, {}),
}


def child(leg, rows, abi):
    """one leg in this process: the block is made on the device, the ctx created, the chain timed"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import benchgen as bg
    import bystro_vcf_amd as bv
    if abi:
        # a parent build checks the version it was made with.  The binding then hands an ABI 9 bvcf_params to an ABI 8
        # library: that works because ABI 9 only APPENDED min_gq / min_dp, which the parent never reads (it copies its
        # own, shorter struct); the parent legs never set a threshold
        bv.ABI_VERSION = abi
    _, kw, _ = LEGS[leg]
    cfg = bg.make_cfg("c5")
    t, nbytes = bg.rows_device(cfg, 0, rows, pad=bv.DEVICE_PAD)
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, **kw)
    ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
    alone, scan, counts = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
    ctx.bench_device([t.data_ptr()], [nbytes], 6)
    flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
    out = {"alone_ms": float(np.median(alone)), "scan_ms": float(np.median(scan)), "in_flight_ms": float(np.mean(flight[3:])),
           "path": ctx.path(), "stream_kernel": ctx.stream_kernel(), "block_MB": nbytes / 1e6, "lines": counts[0]}
    ctx.close()
    print(json.dumps(out))


def run_leg(leg, rows, parent_lib):
    parent, _, env_extra = LEGS[leg]
    env = dict(os.environ, **env_extra)
    for k in ("BVCF_PATH", "BVCF_GEN_STREAM", "BVCF_WIDE"):
        if k not in env_extra:
            env.pop(k, None)
    args = [sys.executable, os.path.abspath(__file__), "--child", leg, "--rows", str(rows)]
    if parent:
        env["BVCF_LIB"] = parent_lib
        args += ["--abi", "8"]
    p = subprocess.run(args, env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, (leg, p.stderr[-600:])
    return json.loads(p.stdout.decode().strip().split("\n")[-1])


def resident(rows, reps, parent_lib):
    legs = [k for k, v in LEGS.items() if parent_lib or not v[0]]
    runs = {k: [] for k in legs}
    for _ in range(reps):
        for k in legs:
            runs[k].append(run_leg(k, rows, parent_lib))
    out = {"rows": rows, "reps": reps}
    for k in legs:
        out[k] = {"alone_ms": statistics.median(r["alone_ms"] for r in runs[k]),
                  "scan_ms": statistics.median(r["scan_ms"] for r in runs[k]),
                  "in_flight_ms": statistics.median(r["in_flight_ms"] for r in runs[k]),
                  "alone_ms_all": [round(r["alone_ms"], 3) for r in runs[k]],
                  "in_flight_ms_all": [round(r["in_flight_ms"], 3) for r in runs[k]],
                  "path": runs[k][0]["path"], "stream_kernel": runs[k][0]["stream_kernel"]}
    out["block_MB"] = runs[legs[0]][0]["block_MB"]
    f = out["filtered"]
    out["filtered_over_census_off"] = f["alone_ms"] / out["census_off"]["alone_ms"]
    out["filtered_over_default_off"] = f["alone_ms"] / out["default_off"]["alone_ms"]
    out["filtered_GBps_alone"] = out["block_MB"] / f["alone_ms"]
    if parent_lib:
        out["filtered_over_parent_census"] = f["alone_ms"] / out["parent_census"]["alone_ms"]
        out["filtered_over_parent_default"] = f["alone_ms"] / out["parent_default"]["alone_ms"]
        out["default_off_over_parent_default_in_flight"] = out["default_off"]["in_flight_ms"] / out["parent_default"]["in_flight_ms"]
        out["default_off_over_parent_default_alone"] = out["default_off"]["alone_ms"] / out["parent_default"]["alone_ms"]
    return out


def cli(exe, args):
    env = dict(os.environ, BVCF_TIMING="json")
    t0 = time.perf_counter()
    p = subprocess.run([exe] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env, timeout=900)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-400:]
    timing = {}
    for ln in p.stderr.decode(errors="replace").split("\n"):
        if ln.startswith("[bvcf timing-json] "):
            timing = json.loads(ln[len("[bvcf timing-json] "):])
    return wall, timing


def e2e(rows, reps, parent_exe):
    sys.path.insert(0, ROOT)
    import benchgen as bg
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_gtf_c5_%d.vcf" % rows)
    cfg = bg.make_cfg("c5")
    if not os.path.exists(path):
        with open(path, "wb") as f:
            f.write(bg.header(cfg))
            for first in range(0, rows, 2_000):
                f.write(bg.rows_host(cfg, first, min(2_000, rows - first)))
    legs = [("plain", EXE, []), ("min_gq_20", EXE, ["--minGQ", "20"])]
    if parent_exe:
        legs.append(("parent_plain", parent_exe, []))
    runs = {k: [] for k, _, _ in legs}
    cli(EXE, ["--in", path])  # (the file into the page cache)
    for _ in range(reps):
        for k, exe, extra in legs:
            runs[k].append(cli(exe, ["--in", path] + extra))
    res = {"rows": rows, "file_MB": os.path.getsize(path) / 1e6, "reps": reps}
    for k, _, _ in legs:
        best = min(runs[k], key=lambda r: r[0])
        res[k] = {"wall_s_median": statistics.median(r[0] for r in runs[k]), "wall_s_all": [round(r[0], 3) for r in runs[k]],
                  "timing_of_fastest": best[1]}
    os.unlink(path)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_288)      # one of bench.py's eight c5 blocks (98 304 rows)
    ap.add_argument("--e2e-rows", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-exe", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--abi", type=int, default=0)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rows, a.abi)
    out = {"resident": resident(a.rows, a.reps, a.parent_lib)}
    if not a.skip_e2e:
        out["e2e_c5"] = e2e(a.e2e_rows, a.reps, a.parent_exe)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
