#!/usr/bin/env python3
"""What does --covar cost?  (not a test): one JSON line.

  chain     a device-resident block of 131 072 configs[2] (c3) rows through the kernel chain with (K, J) = (1, 10) and (4, 10) -- phenotypes of
            |y| < 100 and covariates of |c| < 3 with all six places, every phenotype with the same samples (one mask group):
            the HIP-event medians of the scan's own kernels (bvcf_bench_assoc_kernels) and of the two covariate kernels
            (bvcf_bench_assoc_cov_kernels) over one block; the layout (limbs, blocks, slices) and the records' bytes
  e2e       the CLI's scan-only pass --noOut --pheno --assoc on configs[2] rows from a BGZF file without and with --covar at
            the same (K, J) (the second of two runs each): the host factorises a (J + 3) x (J + 3) matrix per (row, phenotype)

usage: assoc_cov_bench.py [chain|e2e|all] [ROWS]   (e2e rows, default 100 000)"""
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
ROWS = 131_072  # rows of bench.py's configs[2]: at (4, 10) a slot's two arenas stay under their 1 GiB cap with these
CASES = [(1, 10), (4, 10)]


def data(k, j, ns, seed):
    """(Y [k][ns], P [k][ns], C [j][ns], complete [ns]): one sample in twenty without a phenotype, one in fifty incomplete"""
    rng = np.random.default_rng(seed)
    complete = (rng.random(ns) < 0.98).astype(np.uint8)
    present = np.tile(((rng.random(ns) < 0.95) & (complete > 0)).astype(np.uint8), (k, 1))
    return (rng.integers(-10 ** 8, 10 ** 8, size=(k, ns), dtype=np.int64), present,
            rng.integers(-3 * 10 ** 6, 3 * 10 ** 6, size=(j, ns), dtype=np.int64), complete)


def chain(prof="c3"):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS, pad=bv.DEVICE_PAD)
    nh = bg.n_header_fields(cfg)
    out = {"rows": ROWS, "samples": nh - 9}
    for k, j in CASES:
        y, p, c, complete = data(k, j, nh - 9, 2)
        pheno = bv.PhenoTable(y, p)
        covar = bv.CovarTable(c, complete, pheno=pheno)
        ctx = bv.Ctx(nh, max_batch_bytes=nbytes, max_lines=ROWS + 64, n_slots=1, pheno=pheno, covar=covar)
        ctx.bench_device([t.data_ptr()], [nbytes], 2, slots=1)
        own = [ctx.bench_assoc_kernels() for _ in range(5)]
        cov = [ctx.bench_assoc_cov_kernels() for _ in range(5)]
        leg = {"kernel_ms": dict(zip(["k_assoc_list", "k_assoc_gemm", "k_assoc_sparse", "k_assoc_cov_gemm", "k_assoc_cov_sparse"],
                                     [float(x) for x in np.median(np.array(own), axis=0)] + [float(x) for x in np.median(np.array(cov), axis=0)]))}
        t0 = time.perf_counter()
        ctx.submit_device(t.data_ptr(), nbytes)
        ctx.collect()
        leg["submit_collect_ms"] = 1e3 * (time.perf_counter() - t0)
        words = ctx.assoc_cov()
        leg.update(groups=covar.n_groups, limbs=[covar.lc, covar.lcc, covar.lcy], blocks=covar.n_blocks, row_words=covar.row_words,
                   record_rows=int(words.shape[0]), record_MB=words.nbytes / 1e6)
        out["k%d_j%d" % (k, j)] = leg
        ctx.close()
        pheno.close()
        covar.close()
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def decimal(v):
    return (b"-" if v < 0 else b"") + b"%d.%06d" % divmod(abs(int(v)), 10 ** 6)


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_assoc_cov_%d" % rows)
    cfg = bg.make_cfg("c3")
    if not os.path.exists(base + ".bgzf"):
        with open(base + ".bgzf", "wb") as fb:
            fb.write(bgzf.bgzf_compress(bg.header(cfg), eof_marker=False, level=1))
            for first in range(0, rows, 5_000):
                fb.write(bgzf.bgzf_compress(bg.rows_host(cfg, first, min(5_000, rows - first)), eof_marker=False, level=1))
            fb.write(bgzf.bgzf_block(b""))
    res = {"rows": rows}
    names = bg.header(cfg).split(b"\n")[-2].split(b"\t")[9:]
    for k, j in CASES:
        y, p, c, complete = data(k, j, len(names), 3)
        with open(base + ".p", "wb") as f:
            for i, nm in enumerate(names):
                f.write(nm + b"\t" + b"\t".join(decimal(v) if q else b"NA" for v, q in zip(y[:, i], p[:, i])) + b"\n")
        with open(base + ".c", "wb") as f:
            for i, nm in enumerate(names):
                if complete[i]:
                    f.write(nm + b"\t" + b"\t".join(decimal(v) for v in c[:, i]) + b"\n")
        scan = ["--in", base + ".bgzf", "--noOut", "--pheno", base + ".p", "--assoc", base + ".a"]
        for _ in range(2):
            res["no_out_assoc_k%d_s" % k] = cli(scan)
        for _ in range(2):
            res["no_out_covar_k%d_j%d_s" % (k, j)] = cli(scan + ["--covar", base + ".c"])
        for sfx in (".p", ".c", ".a"):
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
