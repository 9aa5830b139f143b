#!/usr/bin/env python3
"""What do --mendel / --mendelErrors cost?  (not a test): one JSON line.

  chain-off   device-resident configs[2] (c3) blocks through the kernel chain without the trios: one block at a time
              and with the library's blocks in flight
  chain-on    the same with bvcf_enable_trios (800 random trios over the block's samples), and the HIP-event time of the
              row index with the two memsets, of k_trio_count, k_trio_scan and k_trio_fill over one block
              (bvcf_bench_trio_kernels), the rows and events of the block, and the bytes of counts and events that cross
              to the host per block
  e2e [ROWS]  the CLI on configs[2] rows from a BGZF file (default 200 000): plain and the QC-only pass
              --noOut --fam --mendel --mendelErrors (the second of two runs each), with the sizes of what it wrote

usage: trio_bench.py chain-off|chain-on|e2e [ROWS]
One leg per process: run the legs in turn, each in a fresh process.  BVCF_LIB / BVCF_EXE name another build (a parent
commit's, for chain-off and the plain e2e leg)."""
import json
import os
import random
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
N_TRIOS = 800
HAS_TRIOS = hasattr(bv.lib, "bvcf_enable_trios")


def random_trios(ns, n, seed=1):
    rng = random.Random(seed)
    trios = []
    for c in sorted(rng.sample(range(ns), n)):
        f, m = rng.sample([s for s in range(ns) if s != c], 2)
        trios.append((c, f, m))
    return trios


def chain(on, prof="c3"):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS, pad=bv.DEVICE_PAD)
    nh = bg.n_header_fields(cfg)
    out = {"trios": N_TRIOS if on else 0, "samples": nh - 9, "lib": os.environ.get("BVCF_LIB", "")}
    ctx = bv.Ctx(nh, max_batch_bytes=nbytes, **({"trios": random_trios(nh - 9, N_TRIOS)} if on else {}))
    if on:  # (unrelated samples under a made-up pedigree: far more events than a real one gives)
        ctx.reserve_trio_events(64 << 20)
    ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
    alone, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
    ctx.bench_device([t.data_ptr()], [nbytes], 6)
    flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
    out["alone_ms"], out["in_flight_ms"] = float(np.median(alone)), float(np.mean(flight[3:]))
    out["alone_ms_all"] = [round(float(x), 4) for x in alone]
    if on:
        ctx.bench_device([t.data_ptr()], [nbytes], 1, slots=1)
        ks = [ctx.bench_trio_kernels() for _ in range(7)]
        ms = np.median(np.array([k[0] for k in ks]), axis=0)
        out["kernel_ms"] = {"row_index_and_memsets": float(ms[0]), "k_trio_count": float(ms[1]), "k_trio_scan": float(ms[2]),
                            "k_trio_fill": float(ms[3])}
        out["rows"], out["events"] = ks[0][1], ks[0][2]
        ctx.submit_device(t.data_ptr(), nbytes)
        ctx.collect()
        info = ctx.trio_info()
        out["d2h_bytes"] = 12 * int(info.n_trios) + 8 * int(info.n_events)
    ctx.close()
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_trio_%d" % rows)
    cfg = bg.make_cfg("c3")
    head = bg.header(cfg)
    if not os.path.exists(base + ".bgzf"):
        with open(base + ".bgzf", "wb") as fb:
            fb.write(bgzf.bgzf_compress(head, eof_marker=False, level=1))
            for first in range(0, rows, 5_000):
                fb.write(bgzf.bgzf_compress(bg.rows_host(cfg, first, min(5_000, rows - first)), eof_marker=False, level=1))
            fb.write(bgzf.bgzf_block(b""))
    names = [ln for ln in head.split(b"\n") if ln.startswith(b"#CHROM")][0].decode().split("\t")[9:]
    names = [n.replace(".", "_") for n in names]
    child = {c: (f, m) for c, f, m in random_trios(len(names), min(N_TRIOS, len(names) // 3))}
    with open(base + ".fam", "w") as f:
        for i, nm in enumerate(names):
            pa, ma = child.get(i, (None, None))
            f.write("F %s %s %s 0 -9\n" % (nm, names[pa] if pa is not None else "0", names[ma] if ma is not None else "0"))
    res = {"rows": rows}
    for _ in range(2):
        res["plain_s"] = cli(["--in", base + ".bgzf"])
    if HAS_TRIOS:
        for _ in range(2):
            res["no_out_mendel_s"] = cli(["--in", base + ".bgzf", "--noOut", "--fam", base + ".fam", "--mendel", base + ".mendel",
                                          "--mendelErrors", base + ".errors"])
        res["mendel_file_MB"] = os.path.getsize(base + ".mendel") / 1e6
        res["errors_file_MB"] = os.path.getsize(base + ".errors") / 1e6
        for ext in (".mendel", ".errors"):
            os.unlink(base + ext)
    os.unlink(base + ".fam")
    return res


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "chain-on"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    if what == "e2e":
        out = {"e2e_c3": e2e(rows)}
    else:
        if what == "chain-on" and not HAS_TRIOS:
            sys.exit("this build of the library has no bvcf_enable_trios")
        out = {"c3": chain(what == "chain-on")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
