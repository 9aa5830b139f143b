#!/usr/bin/env python3
"""What does --pca's solver cost?  (not a test): one JSON line.

bvcf_pca_eigen alone on a GRM-like float32 matrix (tests/pca.py's family, planted groups) at S samples, k = 10: one warm-up
call, then REPS timed calls; the median of the whole call and of each phase (bvcf_bench_pca_eigen: host clocks between the
stream waits the call makes anyway) -- upload + k_pca_expand, the tridiagonalisation, the host's tridiagonal solve, upload +
k_pca_back + download.  Beside it numpy.linalg.eigh of the same matrix in float64 on the host's CPUs, for scale only, and
what the unblocked algorithm must move: 8 S^3 bytes (A22 read by k_pca_symv, read and written by k_pca_rank2, over all
steps), with the rate that makes of the tridiagonalisation's time.  The accuracy ratios of the timed result (tests/pca.py)
are printed too: a fast wrong answer is no answer.

The split of the tridiagonalisation between its four kernels is a kernel trace of the same call:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/pca_bench.py 2504 1 nonumpy

usage: pca_bench.py [S ...] [REPS] [nonumpy]     (S above 64 are sizes, default 2504 8192; REPS at most 64, default 5)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bystro_vcf_amd as bv  # noqa: E402
import pca  # noqa: E402

K = 10
PHASES = ["upload_expand_ms", "tridiagonalise_ms", "host_tridiagonal_ms", "back_transform_ms", "total_ms"]


def one(s, reps, with_numpy):
    A = pca.family("grm", s, markers=min(4 * s + 16, 2048))  # (the time does not depend on the entries; 2 048 markers keep the set-up short)
    lower = pca.lower_f32(A)
    bv.pca_eigen(lower, s, K)  # warm: code objects, the allocator
    runs = []
    for _ in range(reps):
        ms = []
        vals, vecs = bv.pca_eigen(lower, s, K, timings=ms)
        runs.append(ms)
    med = np.median(np.array(runs), axis=0)
    out = dict(zip(PHASES, (float(x) for x in med)))
    out["runs_total_ms"] = [float(r[4]) for r in runs]
    out["launches"] = 4 * (s - 2) + 3 if s > 1 else 1
    out["model_bytes"] = 8.0 * s ** 3
    out["tridiagonalise_TBps_of_model"] = out["model_bytes"] / (out["tridiagonalise_ms"] * 1e-3) / 1e12
    U, u = vecs.T, pca.unit(A)
    out["ratios"] = {"residual": float(np.abs(A @ U - U * vals[None, :]).max()) / u,
                     "orthonormality": float(np.abs(U.T @ U - np.eye(K)).max()) / (s * pca.EPS)}
    if with_numpy:
        t0 = time.perf_counter()
        w = np.linalg.eigh(A)[0]
        out["numpy_eigh_s"] = time.perf_counter() - t0
        out["ratios"]["eigenvalue"] = float(np.abs(vals - w[::-1][:K]).max()) / u
    return out


def main():
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    sizes = [n for n in nums if n > 64] or [2504, 8192]
    reps = ([n for n in nums if n <= 64] or [5])[0]
    print(json.dumps({"k": K, "reps": reps, **{"S%d" % s: one(s, reps, "nonumpy" not in sys.argv) for s in sizes}}))


if __name__ == "__main__":
    main()
