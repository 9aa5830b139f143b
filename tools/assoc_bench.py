#!/usr/bin/env python3
"""What does --pheno / --assoc cost?  (not a test): one JSON line.

  chain     a device-resident configs[2] (c3) block through the kernel chain with the scan off and on -- K = 1 and K = 16
            phenotypes of |y| < 100 with all six places (L1 = 4, L2 = 7): one block at a time and with the library's blocks
            in flight; the HIP-event time of each step of the scan over one block (bvcf_bench_assoc_kernels); the records'
            bytes per block
  e2e       the CLI on configs[2] rows from a BGZF file: plain, and the scan-only pass --noOut --pheno --assoc with K = 1
            and K = 16 (the second of two runs each): the host formats K lines per row there

usage: assoc_bench.py [chain|e2e|all] [ROWS]   (e2e rows, default 100 000)
BVCF_LIB / BVCF_EXE name another build of the library and the CLI (a parent commit's, for the legs without the feature): the
"on" legs and the --assoc runs are then skipped."""
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
HAS_ASSOC = hasattr(bv.lib, "bvcf_set_pheno_table")


def phenotypes(k, ns, seed):
    """(Y [k][ns], P [k][ns]): |y| < 100 with six places, one sample in twenty without a value"""
    rng = np.random.default_rng(seed)
    return rng.integers(-10 ** 8, 10 ** 8, size=(k, ns), dtype=np.int64), (rng.random((k, ns)) < 0.95).astype(np.uint8)


def chain(prof="c3"):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS, pad=bv.DEVICE_PAD)
    nh = bg.n_header_fields(cfg)
    out = {"has_assoc": HAS_ASSOC, "rows": ROWS, "samples": nh - 9}
    legs = [("off", 0)] + ([("k1", 1), ("k16", 16)] if HAS_ASSOC else [])
    for tag, k in legs:
        table = bv.PhenoTable(*phenotypes(k, nh - 9, 2)) if k else None
        ctx = bv.Ctx(nh, max_batch_bytes=nbytes, max_lines=ROWS + 64, **({"pheno": table} if table is not None else {}))
        ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
        alone, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
        ctx.bench_device([t.data_ptr()], [nbytes], 6)
        flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
        out[tag] = {"alone_ms": float(np.median(alone)), "in_flight_ms": float(np.mean(flight[3:]))}
        if table is not None:
            ctx.bench_device([t.data_ptr()], [nbytes], 1, slots=1)
            ks = [ctx.bench_assoc_kernels() for _ in range(5)]
            out[tag]["kernel_ms"] = dict(zip(["k_assoc_list", "k_assoc_gemm", "k_assoc_sparse"],
                                             [float(x) for x in np.median(np.array(ks), axis=0)]))
            t0 = time.perf_counter()
            ctx.submit_device(t.data_ptr(), nbytes)
            ctx.collect()
            out[tag]["submit_collect_ms"] = 1e3 * (time.perf_counter() - t0)
            recs = ctx.assoc()
            out[tag].update(columns=k, n_cols=table.n_cols, l1=table.l1, l2=table.l2, record_rows=int(recs.shape[0]),
                            record_MB=recs.nbytes / 1e6)
            out[tag]["assoc_kernels_ms_per_block"] = out[tag]["alone_ms"] - out["off"]["alone_ms"]
            out[tag]["in_flight_cost_pct"] = 100.0 * (out[tag]["in_flight_ms"] / out["off"]["in_flight_ms"] - 1.0)
        ctx.close()
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_assoc_%d" % rows)
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
    if HAS_ASSOC:
        names = bg.header(cfg).split(b"\n")[-2].split(b"\t")[9:]
        for k in (1, 16):
            y, p = phenotypes(k, len(names), 3)
            with open(base + ".p", "wb") as f:
                for i, nm in enumerate(names):
                    f.write(nm + b"\t" + b"\t".join(b"%d.%06d" % divmod(int(v), 10 ** 6) if v >= 0 and q else b"NA" if not q else
                                                    b"-%d.%06d" % divmod(int(-v), 10 ** 6) for v, q in zip(y[:, i], p[:, i])) + b"\n")
            for _ in range(2):
                res["no_out_assoc_k%d_s" % k] = cli(["--in", base + ".bgzf", "--noOut", "--pheno", base + ".p", "--assoc", base + ".a"])
            res["assoc_file_k%d_MB" % k] = os.path.getsize(base + ".a") / 1e6
            for sfx in (".p", ".a"):
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
