#!/usr/bin/env python3
"""What does --score cost?  (not a test): one JSON line.

  chain     a device-resident configs[2] (c3) block through the kernel chain with the scores off and on -- K = 16 columns of
            five limbs, entries for a tenth of the block's plain SNP rows and for all of them: one block at a time and with
            the library's blocks in flight; the rows the table matched; and the HIP-event time of each score step over one
            block (bvcf_bench_score_kernels)
  e2e       the CLI on configs[2] rows from a BGZF file: plain, and the scoring-only pass --noOut --score (the second of two
            runs each)

usage: score_bench.py [chain|e2e|all] [ROWS]   (e2e rows, default 100 000)
BVCF_LIB / BVCF_EXE name another build of the library and the CLI (a parent commit's, for the legs without the feature): the
"on" legs and the --score runs are then skipped."""
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
K = 16
HAS_SCORE = hasattr(bv.lib, "bvcf_set_score_table")


def snp_loci(text):
    """the TSV locus of every plain SNP line of a block of VCF text"""
    out = []
    for ln in text.split(b"\n"):
        f = ln.split(b"\t", 5)
        if len(f) < 6 or len(f[3]) != 1 or len(f[4]) != 1 or f[4] == b".":
            continue
        chrom = f[0] if len(f[0]) >= 4 and f[0][:1] == b"c" else b"chr" + f[0]
        out.append(b"%s:%s:%s:%s" % (chrom, f[1], f[3], f[4]))
    return list(dict.fromkeys(out))


def weights(n, seed):
    """[n][K] integer weights of five limbs (|w| < 0.5 with all twelve places: a published score's effect sizes)"""
    rng = np.random.default_rng(seed)
    return rng.integers(-499 * 10 ** 9, 499 * 10 ** 9, size=(n, K), dtype=np.int64)


def chain(prof="c3"):
    cfg = bg.make_cfg(prof)
    t, nbytes = bg.rows_device(cfg, 0, ROWS, pad=bv.DEVICE_PAD)
    out = {"has_score": HAS_SCORE, "rows": ROWS, "columns": K}
    loci = snp_loci(bg.rows_host(cfg, 0, ROWS)) if HAS_SCORE else []
    legs = [("off", None)]
    if HAS_SCORE:
        legs += [("tenth", random.Random(1).sample(loci, len(loci) // 10)), ("all", loci)]
    for tag, listed in legs:
        table = bv.ScoreTable(listed, weights(len(listed), 2)) if listed is not None else None
        ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=nbytes, max_lines=ROWS + 64,
                     **({"score": table} if table is not None else {}))
        ctx.bench_device([t.data_ptr()], [nbytes], 4, slots=1)
        alone, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 12, slots=1)
        ctx.bench_device([t.data_ptr()], [nbytes], 6)
        flight, _, _ = ctx.bench_device([t.data_ptr()], [nbytes], 18)
        out[tag] = {"alone_ms": float(np.median(alone)), "in_flight_ms": float(np.mean(flight[3:]))}
        if table is not None:
            ctx.bench_device([t.data_ptr()], [nbytes], 1, slots=1)
            ks = [ctx.bench_score_kernels() for _ in range(5)]
            out[tag]["kernel_ms"] = dict(zip(["k_score_list", "k_score_gemm", "k_score_sparse", "k_score_fold"],
                                             [float(x) for x in np.median(np.array(ks), axis=0)]))
            ctx.score_words(reset=True)
            ctx.submit_device(t.data_ptr(), nbytes)
            ctx.collect()
            out[tag].update(listed=len(listed), limbs=table.n_limbs, matched_rows=ctx.score_words()[4])
            out[tag]["score_kernels_ms_per_block"] = out[tag]["alone_ms"] - out["off"]["alone_ms"]
            out[tag]["in_flight_cost_pct"] = 100.0 * (out[tag]["in_flight_ms"] / out["off"]["in_flight_ms"] - 1.0)
        ctx.close()
    return out


def cli(args):
    t0 = time.perf_counter()
    p = subprocess.run([EXE] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr[-400:]
    return time.perf_counter() - t0


def e2e(rows):
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bvcf_score_%d" % rows)
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
    if HAS_SCORE:
        loci = snp_loci(bg.rows_host(cfg, 0, rows))
        w = weights(len(loci), 3)
        with open(base + ".w", "wb") as f:
            f.write(b"#locus\t" + b"\t".join(b"C%d" % c for c in range(K)) + b"\n")
            for loc, row in zip(loci, w.tolist()):
                f.write(loc + b"\t" + b"\t".join(bv.score_decimal(x) for x in row) + b"\n")
        for _ in range(2):
            res["no_out_score_s"] = cli(["--in", base + ".bgzf", "--noOut", "--score", base + ".w", "--scoreOutput", base + ".s"])
        res["listed"] = len(loci)
        res["score_file_MB"] = os.path.getsize(base + ".w") / 1e6
        for sfx in (".w", ".s"):
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
