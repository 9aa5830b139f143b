#!/usr/bin/env python3
"""What does --keepSamples / --excludeSamples cost, and what does it cost when it is off?  (not a test): one JSON line.

  resident  one device-resident block of bench.py's row model -- c3 (2 504 samples, FORMAT GT) and c5 (GT:DP:GQ) --
            through the kernel chain, one block at a time and with the library's blocks in flight:
              keep10, keep50, keep_all_but_one   this build, a seeded selection of 10 %, 50 %, all but one of the samples
                                                 (the census chain with k_gt_subset; scan_ms is k_gt_subset's own time)
              census_off     this build, no selection, BVCF_PATH=1 (the census chain with k_gt)
              default_off    this build, no selection, the streaming chain the CLI picks for such a file
            and, with --parent-lib (a libbvcf.so of the parent commit), the same two chains of the parent:
              parent_census, parent_default
            Every leg is a fresh child process; the legs are run in turn, --reps times over, so that a drifting box shows
            in all of them alike (medians are reported, all repetitions kept).
  e2e       the CLI over a c5 (or, --e2e-profile c3, a c3) text file plain and with --keepSamples at 10 %
            (BVCF_TIMING=json: the stage split of each run), and the parent's CLI (--parent-exe) over the same file

usage: sample_subset_bench.py [--profiles c3,c5] [--rows N] [--e2e-rows N] [--reps R] [--parent-lib PATH] [--parent-exe PATH]"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
PARENT_ABI = 9  # what a parent build checks bvcf_params.abi_version against

LEGS = {  # name -> (parent build?, share of the samples kept or None, Ctx keywords of a c5 block, environment)
    "keep10": (False, 0.10, {}, {}),
    "keep50": (False, 0.50, {}, {}),
    "keep_all_but_one": (False, -1, {}, {}),
    "census_off": (False, None, {}, {"BVCF_PATH": "1"}),
    "default_off": (False, None, {"path": 3}, {}),
    "parent_census": (True, None, {}, {"BVCF_PATH": "1"}),
    "parent_default": (True, None, {"path": 3}, {}),
}


def kept_samples(ns, share):
    """the seeded selection of a leg: sorted sample indices"""
    rng = random.Random(20261017)
    if share < 0:
        out = rng.randrange(ns)
        return [s for s in range(ns) if s != out]
    return sorted(rng.sample(range(ns), max(1, int(ns * share + 0.5))))


def child(leg, profile, rows, abi):
    """one leg in this process: the block is made on the device, the ctx created, the chain timed"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import benchgen as bg
    import bystro_vcf_amd as bv
    if abi:
        # a parent build checks the version it was made with.  The binding hands it a bvcf_params with sample_keep
        # appended, which the parent never reads (it copies its own, shorter struct); the parent legs never set a mask
        bv.ABI_VERSION = abi
    _, share, kw, _ = LEGS[leg]
    kw = dict(kw)
    if profile != "c5":
        kw.pop("path", None)  # (FORMAT GT: the library's own choice is the streaming chain with k_stream)
    cfg = bg.make_cfg(profile)
    ns = bg.n_header_fields(cfg) - 9
    if share is not None:
        kw["sample_keep"] = kept_samples(ns, share)
    t, nbytes = bg.rows_device(cfg, 0, rows, pad=bv.DEVICE_PAD)
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, **kw)
    ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
    alone, scan, counts = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
    ctx.bench_device([t.data_ptr()], [nbytes], 6)
    flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
    out = {"alone_ms": float(np.median(alone)), "scan_ms": float(np.median(scan)), "in_flight_ms": float(np.mean(flight[3:])),
           "path": ctx.path(), "stream_kernel": ctx.stream_kernel(), "block_MB": nbytes / 1e6, "lines": counts[0],
           "n_keep": ctx.n_samples}
    ctx.close()
    print(json.dumps(out))


def run_leg(leg, profile, rows, parent_lib):
    parent, _, _, env_extra = LEGS[leg]
    env = dict(os.environ, **env_extra)
    for k in ("BVCF_PATH", "BVCF_GEN_STREAM", "BVCF_WIDE"):
        if k not in env_extra:
            env.pop(k, None)
    args = [sys.executable, os.path.abspath(__file__), "--child", leg, "--profiles", profile, "--rows", str(rows)]
    if parent:
        env["BVCF_LIB"] = parent_lib
        args += ["--abi", str(PARENT_ABI)]
    p = subprocess.run(args, env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, (leg, p.stderr[-600:])
    return json.loads(p.stdout.decode().strip().split("\n")[-1])


def resident(profile, rows, reps, parent_lib):
    legs = [k for k, v in LEGS.items() if parent_lib or not v[0]]
    runs = {k: [] for k in legs}
    for _ in range(reps):
        for k in legs:
            runs[k].append(run_leg(k, profile, rows, parent_lib))
    out = {"profile": profile, "rows": rows, "reps": reps}
    for k in legs:
        out[k] = {"alone_ms": statistics.median(r["alone_ms"] for r in runs[k]),
                  "scan_ms": statistics.median(r["scan_ms"] for r in runs[k]),
                  "in_flight_ms": statistics.median(r["in_flight_ms"] for r in runs[k]),
                  "alone_ms_all": [round(r["alone_ms"], 3) for r in runs[k]],
                  "in_flight_ms_all": [round(r["in_flight_ms"], 3) for r in runs[k]],
                  "path": runs[k][0]["path"], "stream_kernel": runs[k][0]["stream_kernel"], "n_keep": runs[k][0]["n_keep"]}
    out["block_MB"] = runs[legs[0]][0]["block_MB"]
    for k in ("keep10", "keep50", "keep_all_but_one"):
        out[k + "_over_census_off"] = out[k]["alone_ms"] / out["census_off"]["alone_ms"]
        out[k + "_over_default_off"] = out[k]["alone_ms"] / out["default_off"]["alone_ms"]
        out[k + "_GBps_alone"] = out["block_MB"] / out[k]["alone_ms"]
        if parent_lib:
            out[k + "_over_parent_census"] = out[k]["alone_ms"] / out["parent_census"]["alone_ms"]
            out[k + "_over_parent_default"] = out[k]["alone_ms"] / out["parent_default"]["alone_ms"]
            out[k + "_over_parent_default_in_flight"] = out[k]["in_flight_ms"] / out["parent_default"]["in_flight_ms"]
    if parent_lib:
        for k, pk in (("census_off", "parent_census"), ("default_off", "parent_default")):
            out[k + "_over_" + pk + "_alone"] = out[k]["alone_ms"] / out[pk]["alone_ms"]
            out[k + "_over_" + pk + "_in_flight"] = out[k]["in_flight_ms"] / out[pk]["in_flight_ms"]
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


def e2e(profile, rows, reps, parent_exe):
    sys.path.insert(0, ROOT)
    import benchgen as bg
    tmp = os.environ.get("TMPDIR", "/tmp")
    path = os.path.join(tmp, "bvcf_subset_%s_%d.vcf" % (profile, rows))
    keep = os.path.join(tmp, "bvcf_subset_%s_keep10.list" % profile)
    cfg = bg.make_cfg(profile)
    hdr = bg.header(cfg)
    if not os.path.exists(path):
        with open(path, "wb") as f:
            f.write(hdr)
            for first in range(0, rows, 2_000):
                f.write(bg.rows_host(cfg, first, min(2_000, rows - first)))
    names = hdr.rstrip(b"\r\n").split(b"\n")[-1].split(b"\t")[9:]
    with open(keep, "wb") as f:
        f.write(b"".join(names[s] + b"\n" for s in kept_samples(len(names), 0.10)))
    legs = [("plain", EXE, []), ("keep10", EXE, ["--keepSamples", keep])]
    if parent_exe:
        legs.append(("parent_plain", parent_exe, []))
    runs = {k: [] for k, _, _ in legs}
    cli(EXE, ["--in", path])  # (the file into the page cache)
    for _ in range(reps):
        for k, exe, extra in legs:
            runs[k].append(cli(exe, ["--in", path] + extra))
    res = {"profile": profile, "rows": rows, "file_MB": os.path.getsize(path) / 1e6, "reps": reps}
    for k, _, _ in legs:
        best = min(runs[k], key=lambda r: r[0])
        res[k] = {"wall_s_median": statistics.median(r[0] for r in runs[k]), "wall_s_all": [round(r[0], 3) for r in runs[k]],
                  "timing_of_fastest": best[1]}
    os.unlink(path)
    os.unlink(keep)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiles", default="c3,c5")
    ap.add_argument("--rows", type=int, default=12_288)      # one of bench.py's eight blocks (98 304 rows)
    ap.add_argument("--e2e-rows", type=int, default=20_000)
    ap.add_argument("--e2e-profile", default="c5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-exe", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--abi", type=int, default=0)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.profiles, a.rows, a.abi)
    out = {"resident": [resident(p, a.rows, a.reps, a.parent_lib) for p in a.profiles.split(",")]}
    if not a.skip_e2e:
        out["e2e"] = e2e(a.e2e_profile, a.e2e_rows, a.reps, a.parent_exe)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
