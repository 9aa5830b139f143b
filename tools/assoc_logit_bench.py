#!/usr/bin/env python3
"""What does --assocModel logistic cost?  (not a test): one JSON line.

  chain     a device-resident block of 131 072 configs[2] (c3) rows -- 65 536 at (4, 10), where a slot's records would pass 1 GiB --
            through the kernel chain with (K, J) = (1, 0), (1, 10) and (4, 10) -- 0/1 phenotypes that lean on the first covariate, covariates of |c| < 3 with all six places: the time
            of the host's null fits, the HIP-event medians of five of the scan's own kernels (bvcf_bench_assoc_kernels) and of
            the two logistic kernels (bvcf_bench_assoc_logit_kernels) over one block; the layout (limbs, blocks) and the
            records' bytes.  tools/assoc_cov_bench.py has --covar's figures for the same block
  e2e       the CLI's scan-only pass --noOut --pheno --covar --assoc on configs[2] rows from a BGZF file without and with
            --assocModel logistic at the same (K, J) (the second of two runs each): the host eliminates on the J + 3 rows of
            the matrix G per (row, phenotype)

usage: assoc_logit_bench.py [chain|e2e|all] [ROWS]   (e2e rows, default 100 000)"""
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
ROWS = 131_072  # rows of bench.py's configs[2], the block of tools/assoc_cov_bench.py
# (K, J, rows): at (4, 10) a row's records are 6.7 KB and a slot's arenas would pass their 1 GiB cap with 131 072 rows: half
CASES = [(1, 0, ROWS), (1, 10, ROWS), (4, 10, ROWS // 2)]


def data(k, j, ns, seed):
    """(Y [k][ns], P [k][ns], C [j][ns], complete [ns]): one sample in twenty without a phenotype, one in fifty incomplete"""
    rng = np.random.default_rng(seed)
    complete = (rng.random(ns) < 0.98).astype(np.uint8)
    present = np.tile(((rng.random(ns) < 0.95) & (complete > 0)).astype(np.uint8), (k, 1))
    c = rng.integers(-3 * 10 ** 6, 3 * 10 ** 6, size=(j, ns), dtype=np.int64)
    lean = 0.1 * c[0] / 3e6 if j else np.zeros(ns)
    y = (rng.random((k, ns)) < 0.3 + 0.05 * np.arange(k)[:, None] + lean[None, :]).astype(np.int64) * 10 ** 6
    return y * present, present, c * complete[None, :], complete


def chain(prof="c3"):
    cfg = bg.make_cfg(prof)
    nh = bg.n_header_fields(cfg)
    out = {"samples": nh - 9}
    for k, j, rows in CASES:
        t, nbytes = bg.rows_device(cfg, 0, rows, pad=bv.DEVICE_PAD)
        y, p, c, complete = data(k, j, nh - 9, 2)
        pheno = bv.PhenoTable(y, p)
        covar = bv.CovarTable(c, complete) if j else None
        t0 = time.perf_counter()
        logit = bv.LogitTable(pheno, covar)
        fit_ms = 1e3 * (time.perf_counter() - t0)
        ctx = bv.Ctx(nh, max_batch_bytes=nbytes, max_lines=rows + 64, n_slots=1, pheno=pheno, logit=logit)
        ctx.bench_device([t.data_ptr()], [nbytes], 2, slots=1)
        own = [ctx.bench_assoc_kernels() for _ in range(5)]
        logit_ms = [ctx.bench_assoc_logit_kernels() for _ in range(5)]
        leg = {"rows": rows, "table_build_ms": fit_ms, "rounds": logit.rounds, "unfitted": logit.n_unfitted,
               "kernel_ms": dict(zip(["k_assoc_list", "k_assoc_gemm", "k_assoc_sparse", "k_assoc_logit_gemm", "k_assoc_logit_sparse"],
                                     [float(x) for x in np.median(np.array(own), axis=0)] + [float(x) for x in np.median(np.array(logit_ms), axis=0)]))}
        t0 = time.perf_counter()
        ctx.submit_device(t.data_ptr(), nbytes)
        ctx.collect()
        leg["submit_collect_ms"] = 1e3 * (time.perf_counter() - t0)
        words = ctx.assoc_logit()
        leg.update(limbs=[logit.lwc, logit.lr, logit.lrc, logit.lwcc], blocks=logit.n_blocks, row_words=logit.row_words,
                   record_rows=int(words.shape[0]), record_MB=words.nbytes / 1e6)
        out["k%d_j%d" % (k, j)] = leg
        ctx.close()
        for tb in (pheno, covar, logit):
            if tb is not None:
                tb.close()
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def decimal(v):
    return (b"-" if v < 0 else b"") + b"%d.%06d" % divmod(abs(int(v)), 10 ** 6)


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_assoc_logit_%d" % rows)
    cfg = bg.make_cfg("c3")
    if not os.path.exists(base + ".bgzf"):
        with open(base + ".bgzf", "wb") as fb:
            fb.write(bgzf.bgzf_compress(bg.header(cfg), eof_marker=False, level=1))
            for first in range(0, rows, 5_000):
                fb.write(bgzf.bgzf_compress(bg.rows_host(cfg, first, min(5_000, rows - first)), eof_marker=False, level=1))
            fb.write(bgzf.bgzf_block(b""))
    res = {"rows": rows}
    names = bg.header(cfg).split(b"\n")[-2].split(b"\t")[9:]
    for k, j, _ in CASES:
        y, p, c, complete = data(k, j, len(names), 3)
        with open(base + ".p", "wb") as f:
            for i, nm in enumerate(names):
                f.write(nm + b"\t" + b"\t".join(decimal(v) if q else b"NA" for v, q in zip(y[:, i], p[:, i])) + b"\n")
        with open(base + ".c", "wb") as f:
            for i, nm in enumerate(names):
                if complete[i]:
                    f.write(nm + b"\t" + b"\t".join(decimal(v) for v in c[:, i]) + b"\n")
        scan = ["--in", base + ".bgzf", "--noOut", "--pheno", base + ".p", "--assoc", base + ".a"] + (["--covar", base + ".c"] if j else [])
        for _ in range(2):
            res["no_out_linear_k%d_j%d_s" % (k, j)] = cli(scan)
        for _ in range(2):
            res["no_out_logistic_k%d_j%d_s" % (k, j)] = cli(scan + ["--assocModel", "logistic"])
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
